"""The audits against the live list with timing slack on the GPU (pmaf_evaluate_paths_slack / pmaf_select_clear_slack,
k_obs_slack_audit<false|true> of csrc/pmaf_k_obslack.hip) through the C-ABI against tests/obstacle_slack_reference.py at
TOLERANCE 0: integers equal, doubles bit-equal. The reference is fed the handle's own paths(), n_points and costs(), the
live list and the tracks as they were uploaded, and takes its dot association from pmaf_eval_order(), so the file passes
unchanged under PMAF_VARIANT=rassoc. tests/test_obstacle_slack_audit.py validates the reference on the CPU and shows
that the shapes are sensitive to every rule of the contract.

Shapes, chosen where the kernel can go wrong: (P, N, M, cap) = (1, 5, 1, 9), (1, 5, 3, 70), (2, 16, 59, 70), (2, 16, 60, 9)
(60 field obstacles is the most a tracked handle can have), the multi-tile untracked (2, 5, 66, 9), and one population
with L = 0 beside a tracked one. The handle, its tracks and its live list are tests/test_tracked_audit_gpu.py's Case."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conftest
import field_track_reference as fref
import obstacle_slack_reference as ref
from test_tracked_audit_gpu import Case, INT32_MAX, INT_KEYS, DBL_KEYS, ERR_INVALID, ERR_STATE, _same_bits, _state, _tracks, build_scene

pytestmark = pytest.mark.gpu

ROOT = conftest.ROOT
AUDIT_INTS = ("step", "obstacle_step", "obstacle", "first_violation")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("PMAF_SUM", "PMAF_FORCE_GENERIC", "PMAF_PLAIN_STEP", "PMAF_MW", "PMAF_W64_SLICE"):
        monkeypatch.delenv(k, raising=False)


class SlackCase(Case):
    """Case with the slacked calls held to the reference, and a second live list whose trailing sphere MOVES: it reaches
    agent 1's path point k*, half way, at the obstacles' index k* + 2"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.moving = self.live.copy()
        v = np.array([0.9, -1.3, 0.7])
        for p in range(self.P):
            k = int(self.n[p][1]) // 2
            at = np.asarray(self.paths[p][1][k], dtype=np.float64)
            for _ in range(k + 2):
                at = at - v * self.sc["dt"]
            self.moving[p, -1] = list(at) + list(v) + [0.02]

    def slack_select(self, margin, horizon, late, early, first=None, skip=False, prev=None, live=None, what=""):
        """one pmaf_select_clear_slack call (adopt = 0) against the reference; returns the call's dict as arrays [P]"""
        live = self.live if live is None else live
        arg, f = self._first(first)
        got = self.pl.select_clear_slack(live, margin, horizon, late, early, prev=prev, first=arg, skip_trailing=skip)
        got = {k: np.asarray(v).reshape(self.P) for k, v in got.items()}
        pv = None if prev is None else np.broadcast_to(np.asarray(prev), (self.P,)).tolist()
        want = ref.select_clear(self.paths, self.n, live.tolist(), self.attached, f, self.costs, self.sc["dt"], self.sc["radius"],
                                margin, horizon, skip, late, early, self.order, pv)
        tag = "%s select margin %r horizon %r band (%r, %r) first %r skip %r prev %r" % (what, margin, horizon, late, early, first,
                                                                                       skip, prev)
        print(tag, "got", {k: v.tolist() for k, v in got.items()})
        for k in INT_KEYS:
            np.testing.assert_array_equal(got[k], np.asarray(want[k]), err_msg=k + " " + tag)
        for k in DBL_KEYS:
            _same_bits(got[k], want[k], k + " " + tag)
        return got

    def slack_audit(self, margin, late, early, first=None, live=None, what=""):
        """one pmaf_evaluate_paths_slack call against the reference; returns the call's dict as arrays [P][N]"""
        live = self.live if live is None else live
        arg, f = self._first(first)
        got = self.pl.evaluate_paths_slack(live, margin, late, early, first=arg)
        got = {k: np.asarray(v).reshape(self.P, self.N) for k, v in got.items()}
        want = ref.audit(self.paths, self.n, live.tolist(), self.attached, f, self.sc["dt"], self.sc["radius"], margin, late,
                         early, self.order)
        tag = "%s audit margin %r band (%r, %r) first %r" % (what, margin, late, early, first)
        print(tag, "clearance", got["clearance"].tolist(), "step", got["step"].tolist(), "obstacle_step",
              got["obstacle_step"].tolist(), "fv", got["first_violation"].tolist())
        for k in AUDIT_INTS:
            np.testing.assert_array_equal(got[k], np.asarray(want[k]), err_msg=k + " " + tag)
        _same_bits(got["clearance"], want["clearance"], "clearance " + tag)
        return got


# (P, N, M, cap)
SHAPES = [(1, 5, 1, 9), (1, 5, 3, 70), (2, 16, 59, 70), (2, 16, 60, 9)]
_ids = lambda s: "P%d-N%d-M%d-cap%d" % tuple(s[:4])


def _bands(cap, big):
    """the bands; (cap + 5, cap + 5) -- clamped to (cap, cap) -- where the reference's 2 cap indices per point stay cheap"""
    return [(0, 0), (1, 0), (0, 1), (2, 3)] + ([(cap + 5, cap + 5)] if big else [])


# ---- 1. fails without the feature: the constructed scenes ----------------------------------------------------------------
def _far_list(c):
    """the case's live list with field obstacle 0 small, at rest and far away, and the trailing obstacle out of the way"""
    live = c.live.copy()
    live[:, 0] = [50.0, 50.0, 50.0, 0.0, 0.0, 0.0, 0.01]
    live[:, -1] = [100.0, 100.0, 100.0, 0.0, 0.0, 0.0, 0.02]
    return live


@pytest.mark.parametrize("shape", [(1, 5, 3, 70), (2, 16, 59, 70)], ids=_ids)
def test_an_arm_that_runs_late_is_held_to_the_obstacle_that_crosses_behind_it(pmaf, scenes, hip_lib, shape):
    """Obstacle 0 rests far away in the live list; its track crosses the cheapest clear agent's path point x_{k*} at the
    obstacles' index k* + 3, three steps after the agent has passed. pmaf_select_clear_tracked calls the agent clear and
    picks it; pmaf_select_clear_slack with late = 3 does not, late = 2 and early = 3 still do. The mirror with early: the
    predictor's obstacle reaches x_{k*} two indices EARLY (index k* - 2): early = 2 rejects, late = 3 does not."""
    c = SlackCase(pmaf, scenes, hip_lib, *shape)
    P, cap = c.P, c.cap
    try:
        pl, dt = c.pl, c.sc["dt"]
        far = _far_list(c)
        # The path's points lie millimetres apart, far inside the spheres: the margin is set so that only a hit of the path
        # point itself counts. An exact hit gives c = -(radius + 0.01); the margin lies half the distance to the star
        # agent's nearest other path point above that.
        exact = -(c.sc["radius"] + 0.01)
        star = np.asarray(pl.select_clear(far, exact, cap)["pick"]).reshape(P).tolist()
        w = [min(c.n[p][star[p]], cap) for p in range(P)]
        assert min(w) >= 8
        kstar = [w[p] // 2 for p in range(P)]
        dmin = []
        for p in range(P):
            x = np.asarray(c.paths[p][star[p]][:c.n[p][star[p]]])
            d = np.linalg.norm(x - x[kstar[p]], axis=1)
            dmin.append(float(np.delete(d, kstar[p]).min()))
        assert min(dmin) > 1e-4, dmin
        margin = exact + 0.5 * min(dmin)
        plain = {k: np.asarray(v).reshape(P) for k, v in pl.select_clear(far, margin, cap).items()}
        assert (plain["rule"] == 1).all() and plain["pick"].tolist() == star and plain["first_violation"].tolist() == w
        for shift, hits, misses in ((3, (3, 0), ((2, 0), (0, 3))), (-2, (0, 2), ((3, 0), (0, 1)))):
            tracks = []
            for p in range(P):
                t = fref.straight_lines(far[p], dt, cap + 5)
                t[kstar[p] + shift, 0, 0:3] = c.paths[p][star[p]][kstar[p]]
                tracks.append(t)
            c.attach(tracks)
            un = {k: np.asarray(v).reshape(P) for k, v in pl.select_clear_tracked(far, margin, cap).items()}
            np.testing.assert_array_equal(un["pick"], plain["pick"])       # step against step the agent is clear
            assert (un["rule"] == 1).all()
            got = c.slack_select(margin, cap, hits[0], hits[1], live=far, what="shift %d" % shift)
            kept = c.slack_select(margin, cap, hits[0], hits[1], live=far, prev=star, what="shift %d, prev = the agent" % shift)
            audit = pl.evaluate_paths_slack(far, margin, hits[0], hits[1])
            audit = {k: np.asarray(v).reshape(P, c.N) for k, v in audit.items()}
            for p in range(P):
                for r in (got, kept):
                    assert not (r["rule"][p] in (0, 1) and r["pick"][p] == star[p])
                a = star[p]
                assert audit["clearance"][p][a] == exact
                assert (audit["step"][p][a], audit["obstacle_step"][p][a], audit["obstacle"][p][a]) == (kstar[p], kstar[p] + shift, 0)
                assert audit["first_violation"][p][a] == kstar[p]          # the ARM'S step
            for late, early in misses:
                r = c.slack_select(margin, cap, late, early, live=far, prev=star, what="shift %d, too little slack" % shift)
                assert (r["rule"] == 0).all() and r["pick"].tolist() == star
        c.slack_audit(margin, 0, 2, live=far, what="the early obstacle")
    finally:
        c.close()


# ---- 2. (0, 0): device against device --------------------------------------------------------------------------------------
def _zero_band_against_the_unslacked_calls(c, live, margin, horizon, first=None, skip=False, prev=None):
    pl = c.pl
    a = pl.select_clear_tracked(live, margin, horizon, prev=prev, first=first, skip_trailing=skip)
    b = pl.select_clear_slack(live, margin, horizon, 0, 0, prev=prev, first=first, skip_trailing=skip)
    for k in INT_KEYS + DBL_KEYS:
        _same_bits(np.asarray(b[k], dtype=np.float64), np.asarray(a[k], dtype=np.float64), k)
    a = pl.evaluate_paths_tracked(live, margin, first=first)
    b = pl.evaluate_paths_slack(live, margin, 0, 0, first=first)
    for k in a:
        _same_bits(np.asarray(b[k], dtype=np.float64), np.asarray(a[k], dtype=np.float64), k)
    np.testing.assert_array_equal(b["obstacle_step"], b["step"])


@pytest.mark.parametrize("shape", SHAPES + [(2, 5, 66, 9)], ids=_ids)
def test_zero_slack_is_the_unslacked_calls_bit_for_bit(pmaf, scenes, hip_lib, shape):
    """(late, early) = (0, 0) against pmaf_select_clear_tracked and pmaf_evaluate_paths_tracked on the same handle: without
    tracks (also on more than 64 obstacles: several tiles), and with tracks of every length read from every offset"""
    c = SlackCase(pmaf, scenes, hip_lib, *shape)
    try:
        for live in (c.live, c.moving):
            for margin, horizon in ((0.0, c.cap), (0.05, 3), (3.0, c.cap + 5), (-0.5, 1)):
                _zero_band_against_the_unslacked_calls(c, live, margin, horizon, prev=[1] * c.P)
        if c.M <= 60:
            for name, first in (("L1", 0), ("L2", 1), ("Lcap", "L-1"), ("Lcap+5", 1), ("short", INT32_MAX), ("short", 0)):
                t = _tracks(c, name)
                c.attach(t)
                f = np.asarray([fref.resolve_first(first, len(t[p])) for p in range(c.P)], dtype=np.int32)
                for margin, horizon, skip in ((0.0, c.cap, False), (0.1, 5, True), (0.02, 2, False)):
                    _zero_band_against_the_unslacked_calls(c, c.moving, margin, horizon, first=f, skip=skip, prev=[2] * c.P)
            c.attach(_tracks(c, "short"), [2] * c.P)
            _zero_band_against_the_unslacked_calls(c, c.live, 0.0, c.cap)          # first = NULL: the handle's offsets
    finally:
        c.close()


# ---- 3. bands, horizons, lengths, offsets against the reference ------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_bands_lengths_offsets_against_the_reference(pmaf, scenes, hip_lib, shape):
    c = SlackCase(pmaf, scenes, hip_lib, *shape)
    P, cap = c.P, c.cap
    big = c.N * c.M * cap <= 5 * 3 * 70
    try:
        # no tracks attached: every obstacle on the list's chain, at rest (the trailing one) and moving
        for late, early in _bands(cap, big) if big else [(2, 3)]:
            c.slack_audit(0.02, late, early, live=c.moving, what="no tracks")
        c.slack_select(0.02, cap, 2, 3, live=c.moving, prev=1, what="no tracks")
        # track lengths 1, 2, cap, cap + 5 and one that ends mid-path (the held end); offsets 0, 1, L-1, L+3, INT32_MAX
        # (the selection's window audit is the same kernel on min(n, horizon) points: where the plain-Python reference of
        # the whole paths costs seconds -- 16 agents x 70 points x 60 obstacles -- the selection runs on a window of 12)
        cases = (("L1", 0, (2, 3)), ("L2", 1, (1, 0)), ("Lcap", "L-1", (0, 1)), ("Lcap+5", 1, (2, 3)), ("short", "L+3", (2, 3)),
                 ("short", INT32_MAX, (0, 1)), ("Lcap", 0, (cap + 5, cap + 5) if big else (1, 0)), ("short", 1, (2, 3)))
        for i, (name, first, (late, early)) in enumerate(cases):
            t = _tracks(c, name)
            f = [fref.resolve_first(first, len(t[p])) for p in range(P)]
            c.attach(t)
            c.slack_select(0.0, cap + 5 if big else 12, late, early, first=f, prev=1, live=c.moving, what=name)
            if big or i in (3, 4):
                c.slack_audit(0.0, late, early, first=f, live=c.moving, what=name)
        # first = NULL after pmaf_set_obstacle_track_offset; an explicit offset then overrides the handle's
        c.attach(_tracks(c, "short"), [2] * P)
        a = c.slack_select(0.0, cap, 2, 3, what="handle offset")
        b = c.slack_select(0.0, cap, 2, 3, first=2, what="the same offset given")
        for k in INT_KEYS + DBL_KEYS:
            _same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), k)
        c.slack_select(0.0, cap, 2, 3, first=0, what="explicit 0 over the handle's 2")
        _, first_now = c.pl.get_obstacle_tracks()
        assert list(first_now) == [2] * P          # the call's offsets did not become the handle's
        # the rules: nobody clear (2, the fallback); everybody clear (1, the cheapest; 0, the previous pick kept)
        r = c.slack_select(3.0, cap, 1, 1)
        assert (r["rule"] == 2).all() and (r["n_clear"] == 0).all()
        r = c.slack_select(-0.5, cap, 1, 1)
        assert (r["rule"] == 1).all() and (r["n_clear"] == c.N).all()
        r = c.slack_select(-0.5, cap, 1, 1, prev=r["pick"].tolist())
        assert (r["rule"] == 0).all()
        w = c.slack_select(0.0, cap, 2, 0, skip=False, live=c.moving)
        s = c.slack_select(0.0, cap, 2, 0, skip=True, live=c.moving)
        assert (s["n_clear"] >= w["n_clear"]).all()
    finally:
        c.close()


@pytest.mark.parametrize("horizon", [1, 2, 3, 5, 9])
def test_windows_of_fewer_than_two_indices_per_wave(pmaf, scenes, hip_lib, horizon):
    """the kernel splits the w + late indices of the obstacles over four waves in quarters: horizons 1, 2, 3, 5 with small
    slacks leave waves without an index or with one; every band, with and without tracks, both trailing settings"""
    c = SlackCase(pmaf, scenes, hip_lib, 2, 5, 3, 9)
    try:
        assert all(n >= 5 for row in c.n for n in row)
        for late, early in _bands(c.cap, True):
            c.slack_select(0.05, horizon, late, early, prev=[1, 3], live=c.moving, what="no tracks")
        for name, first in (("Lcap", 0), ("short", 1), ("L2", INT32_MAX)):
            t = _tracks(c, name)
            c.attach(t)
            f = [fref.resolve_first(first, len(t[p])) for p in range(c.P)]
            for late, early in _bands(c.cap, True):
                for skip in (False, True):
                    got = c.slack_select(0.05, horizon, late, early, first=f, skip=skip, prev=[1, 3], live=c.moving, what=name)
                    assert (got["first_violation"] <= horizon).all()
    finally:
        c.close()


def test_more_than_one_tile_of_obstacles(pmaf, scenes, hip_lib):
    """66 obstacles (a handle that can have no tracks): two tiles of 64 lanes, the second with two audited lanes; the
    trailing obstacle, j = 66, moves through agent 1's path"""
    c = SlackCase(pmaf, scenes, hip_lib, 2, 5, 66, 9)
    try:
        for late, early in _bands(c.cap, False) + [(14, 14)]:
            a = c.slack_audit(0.02, late, early, live=c.moving)
            c.slack_select(0.02, 7, late, early, prev=[0, 2], live=c.moving)
        k = [c.n[p][1] // 2 for p in range(2)]
        hit = c.slack_audit(0.0, 2, 0, live=c.moving)
        for p in range(2):
            assert (hit["step"][p][1], hit["obstacle_step"][p][1], hit["obstacle"][p][1]) == (k[p], k[p] + 2, 66)
        # a list at rest: the unslacked calls' bits for every slack
        rest = c.live.copy()
        rest[:, :, 3:6] = 0.0
        want = c.pl.evaluate_paths(rest, 0.02)
        sel = c.pl.select_clear(rest, 0.02, 7, prev=[0, 2])
        for late, early in ((2, 3), (0, 1), (14, 14)):
            got = c.pl.evaluate_paths_slack(rest, 0.02, late, early)
            for key in ("clearance", "step", "obstacle", "first_violation"):
                _same_bits(np.asarray(got[key], dtype=np.float64), np.asarray(want[key], dtype=np.float64), key)
            s = c.pl.select_clear_slack(rest, 0.02, 7, late, early, prev=[0, 2])
            for key in INT_KEYS + DBL_KEYS:
                _same_bits(np.asarray(s[key], dtype=np.float64), np.asarray(sel[key], dtype=np.float64), key)
    finally:
        c.close()


def test_one_population_without_tracks_beside_a_tracked_one(pmaf, scenes, hip_lib):
    c = SlackCase(pmaf, scenes, hip_lib, 2, 5, 3, 70)
    try:
        for given in ([c.tracks[0]["Lcap"], None], [None, c.tracks[1]["short"]]):
            c.attach(given, [1, 2])
            for late, early in ((2, 3), (0, 1)):
                c.slack_select(0.05, c.cap, late, early, prev=[0, 2], live=c.moving)
                c.slack_audit(0.0, late, early, live=c.moving)
            c.slack_select(0.0, 7, 2, 3, first=[3, 0], skip=True, live=c.moving)
    finally:
        c.close()


def test_nothing_grows_with_either_slack(pmaf, scenes, hip_lib):
    c = SlackCase(pmaf, scenes, hip_lib, 2, 16, 59, 70)
    try:
        c.attach(_tracks(c, "short"), [1, 1])
        bands = [(0, 0), (1, 0), (0, 1), (2, 3), (5, 5), (75, 75)]
        res = {}
        for b in bands:
            a = c.pl.evaluate_paths_slack(c.moving, 0.05, b[0], b[1])
            s = c.pl.select_clear_slack(c.moving, 0.05, 50, b[0], b[1])
            res[b] = (np.asarray(a["clearance"]), np.asarray(a["first_violation"]), np.asarray(s["n_clear"]))
        for small in bands:
            for big in bands:
                if big[0] >= small[0] and big[1] >= small[1]:
                    for x, y in zip(res[small], res[big]):
                        assert (y <= x).all(), (small, big)
    finally:
        c.close()


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smallest_k_then_l_then_j(pmaf, scenes, hip_lib):
    """c = -(radius + r) is the least a pair can give. Obstacle 0's track is at agent 0's point 6 at index 8 and at its
    point 7 at index 7: the pairs (6, 8) and (7, 7) tie and (6, 8) wins although index 7 comes first. And the trailing
    obstacle rests at agent 2's point 5 where obstacle 0's track is at index 4: (5, 4, 0) and (5, l, M) tie for every l
    of the band and the smallest l wins, then the smaller j."""
    c = SlackCase(pmaf, scenes, hip_lib, 1, 5, 3, 70)
    try:
        assert c.n[0][0] >= 9 and c.n[0][2] >= 9
        live = c.live.copy()
        live[0, 0, 6] = 0.03
        live[0, -1] = list(c.paths[0][2][5]) + [0.0, 0.0, 0.0, 0.03]
        t = np.array(c.tracks[0]["Lcap"], copy=True)
        t[8, 0, 0:3] = c.paths[0][0][6]
        t[7, 0, 0:3] = c.paths[0][0][7]
        t[4, 0, 0:3] = c.paths[0][2][5]
        c.attach([t])
        got = c.slack_audit(0.0, 2, 1, live=live)
        assert got["clearance"][0][0] == -(c.sc["radius"] + 0.03) == got["clearance"][0][2]
        assert (got["step"][0][0], got["obstacle_step"][0][0], got["obstacle"][0][0]) == (6, 8, 0)
        assert (got["step"][0][2], got["obstacle_step"][0][2], got["obstacle"][0][2]) == (5, 4, 0)
        got = c.slack_audit(0.0, 2, 0, live=live)       # index 4 is out of the band: the trailing obstacle, smallest l
        assert (got["step"][0][2], got["obstacle_step"][0][2], got["obstacle"][0][2]) == (5, 5, 3)
        c.slack_select(0.0, c.cap, 2, 1, live=live)
    finally:
        c.close()


# ---- 5. NULL outputs, errors ---------------------------------------------------------------------------------------------------
def test_optional_outputs_may_be_null_and_the_error_returns(pmaf, scenes, hip_lib):
    c = SlackCase(pmaf, scenes, hip_lib, 2, 5, 3, 9)
    try:
        pl, L, h = c.pl, hip_lib, c.pl._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        obs = np.ascontiguousarray(c.live, dtype=np.float64)
        # a handle without tracks: an offset is refused, a negative one first; NULL is the list's line
        for call in (lambda **kw: pl.select_clear_slack(c.live, 0.0, 9, 1, 1, first=kw.get("first")),
                     lambda **kw: pl.evaluate_paths_slack(c.live, 0.0, 1, 1, first=kw.get("first"))):
            with pytest.raises(pmaf.PmafError) as e:
                call(first=[0, 0])
            assert e.value.code == ERR_STATE, str(e.value)
            with pytest.raises(pmaf.PmafError) as e:
                call(first=[0, -1])
            assert e.value.code == ERR_INVALID, str(e.value)
            call()
        c.attach(_tracks(c, "L2"), [1, 1])
        full = c.slack_select(0.0, 9, 2, 3, first=1)
        pick = np.full(2, -7, dtype=np.int32)
        f1 = np.array([1, 1], dtype=np.int32)
        for first in (None, f1.ctypes.data_as(ip)):
            assert L.pmaf_select_clear_slack(h, obs.ctypes.data_as(dp), first, 0.0, 9, 0, 2, 3, None, 0, pick.ctypes.data_as(ip),
                                             None, None, None, None, None) == 0
            np.testing.assert_array_equal(pick, full["pick"])
        assert L.pmaf_select_clear_slack(h, obs.ctypes.data_as(dp), None, 0.0, 9, 0, 2, 3, None, 0, None, None, None, None, None,
                                         None) == ERR_INVALID
        clr = np.zeros((2, 5))
        assert L.pmaf_evaluate_paths_slack(h, obs.ctypes.data_as(dp), f1.ctypes.data_as(ip), 0.0, 2, 3, clr.ctypes.data_as(dp),
                                           None, None, None, None) == 0
        _same_bits(clr, c.slack_audit(0.0, 2, 3, first=1)["clearance"], "clearance alone")
        assert L.pmaf_evaluate_paths_slack(h, obs.ctypes.data_as(dp), None, 0.0, 2, 3, None, None, None, None, None) == ERR_INVALID
        # the slacks
        for late, early in ((-1, 0), (0, -1), (-2 ** 31, 3)):
            with pytest.raises(pmaf.PmafError) as e:
                pl.select_clear_slack(c.live, 0.0, 9, late, early)
            assert e.value.code == ERR_INVALID and "late" in str(e.value), str(e.value)
            with pytest.raises(pmaf.PmafError) as e:
                pl.evaluate_paths_slack(c.live, 0.0, late, early)
            assert e.value.code == ERR_INVALID and "late" in str(e.value), str(e.value)
        a = pl.evaluate_paths_slack(c.live, 0.0, INT32_MAX, INT32_MAX)       # clamped to max_prediction_steps on the host
        b = pl.evaluate_paths_slack(c.live, 0.0, c.cap, c.cap)
        for k in a:
            _same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), k)
        # everything else as in the tracked calls
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_slack(c.live, float("nan"), 9, 1, 1)
        assert e.value.code == ERR_INVALID and "range" in str(e.value), str(e.value)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_slack(c.live, 0.0, 0, 1, 1)
        assert e.value.code == ERR_INVALID and "horizon" in str(e.value)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_slack(c.live, 0.0, 9, 1, 1, prev=[5, 0])
        assert e.value.code == ERR_INVALID and "prev_idx" in str(e.value)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_slack(c.live, 0.0, 9, 1, 1, first=[3, -1])
        assert e.value.code == ERR_INVALID and "first" in str(e.value)
        # (the refusal of a handle whose tick was abandoned is select_clear's own guard, require_drained, which this call
        # goes through unchanged: tests/test_tracked_audit_gpu.py::test_refused_after_an_abandoned_tick holds it)
    finally:
        c.close()


# ---- 6. state --------------------------------------------------------------------------------------------------------------------
def test_adoption_steers_the_real_step(pmaf, scenes, hip_lib):
    """adopt = 1: pmaf_get_best names the pick, and the next pmaf_move_real is the one of a handle that selected with
    adopt = 0 and adopted the pick through pmaf_adopt_best"""
    cs = [SlackCase(pmaf, scenes, hip_lib, 2, 5, 3, 70, True) for _ in range(2)]
    try:
        picks = []
        for i, c in enumerate(cs):
            c.attach(_tracks(c, "Lcap"), [1, 2])
            before = np.asarray(c.pl.best()[1]).copy()
            r = c.pl.select_clear_slack(c.moving, 0.0, c.cap, 2, 3, prev=[1, 1], adopt=(i == 0))
            pick = np.asarray(r["pick"]).reshape(2)
            picks.append(pick)
            if i == 0:
                np.testing.assert_array_equal(c.pl.best()[1], pick + 1)
            else:
                np.testing.assert_array_equal(c.pl.best()[1], before)
                c.pl.adopt_best(pick)
            c.pl.move_real(c.moving, c.sc["dt"], 1, pick)
        np.testing.assert_array_equal(picks[0], picks[1])
        a, b = _state(cs[0].pl), _state(cs[1].pl)
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a[3], b[3]):
            _same_bits(x, y, "the real agent after the step")
    finally:
        for c in cs:
            c.close()


def test_calls_without_adoption_between_ticks_change_nothing(pmaf, scenes, hip_lib):
    """six closed-loop ticks with the offset one further in front of each, with and without slacked audits (adopt = 0, own
    offsets) in between: bit-identical"""
    sc = build_scene(scenes, 5, 3, 70)
    runs = []
    tracks = None
    for audits in (False, True):
        pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
        try:
            pl.set_initial_position(sc["start"])
            pl.rollout()
            paths, n = pl.paths()
            if tracks is None:
                tracks = fref.tracks_for(sc, np.asarray(paths)[0], int(n[0]))["sweep"]
            pl.set_initial_position(sc["start"])
            pl.set_obstacle_tracks(tracks)
            rec = []
            for t in range(6):
                pl.set_obstacle_track_offset(t)
                b = pl.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
                rec.append((int(b), pl.last_next_pos.copy(), pl.last_next_vel.copy()))
                if audits:
                    live = scenes.advance_live_obstacles(sc["obstacles"])
                    r = pl.select_clear_slack(live, 0.05, 50 if t % 2 else 1000, t % 4, 3 - t % 4, prev=int(b),
                                              first=None if t % 3 else t + 4)
                    assert 0 <= r["pick"] < pl.N
                    pl.evaluate_paths_slack(live, 0.05, 2, t, first=t)
                    _, first_now = pl.get_obstacle_tracks()
                    assert list(first_now) == [t]
            pl.stop()
            rec.append((0, np.asarray(pl.paths()[0]).copy(), np.asarray(pl.real_known()[1]).copy()))
            runs.append(rec)
        finally:
            pl.close()
    for (b0, p0, v0), (b1, p1, v1) in zip(*runs):
        assert b0 == b1
        _same_bits(p1, p0, "set-point position / paths")
        _same_bits(v1, v0, "set-point velocity / real rotation vectors")


# ---- 7. the facade ---------------------------------------------------------------------------------------------------------------
def test_facade_slack_tick_equals_the_c_abi_sequence(pmaf, scenes, tmp_path, hip_lib):
    """tests/cpp/facade_slack_tick.cpp runs CfManager::planTickAudited(tracked = true, late, early) over 5 ticks with
    advanceObstacleTracks in between, then evaluatePathsSlack and selectClearSlack; every figure it prints equals the same
    calls made through the binding"""
    N, cap, ticks, L, margin, horizon, late, early = 12, 101, 5, 40, 0.05, 60, 3, 2
    sc = scenes.static1_scene(N, cap - 1)
    rvf = tmp_path / "rv.bin"
    np.ascontiguousarray(sc["random_vecs"]).tofile(rvf)
    exe = conftest.exe(os.path.join(ROOT, "tests", "cpp", "facade_slack_tick"))
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    out = subprocess.run([exe, str(N), str(cap), str(ticks), str(rvf), str(L), repr(margin), str(horizon), str(late), str(early)],
                         capture_output=True, check=True, env=conftest.binary_env(pmaf)).stdout.decode()
    lines = out.strip().split("\n")
    assert len(lines) == ticks
    k = np.arange(L, dtype=np.float64)
    t6 = np.zeros((L, 9, 6))
    t6[:, :, 0:3] = sc["obstacles"][None, :9, 0:3]
    t6[:, :, 0] = sc["obstacles"][None, :9, 0] + 0.0005 * k[:, None]
    t6[:, :, 3:6] = np.stack([np.full(9, 0.05), np.zeros(9), 0.01 * np.arange(9)], axis=1)[None]
    t6[:, 0, 0:3] = np.stack([-0.6 + 0.002 * k, 0.3 - 0.001 * k, np.full(L, 0.75)], axis=1)
    t6[:, 0, 3:6] = [0.2, -0.1, 0.0]
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        pl.set_obstacle_tracks(t6)
        pl.set_obstacle_track_offset(2)
        pl.start()
        prev = None
        differs = False
        for t in range(ticks):
            if t > 0:
                pl.stop()
                pl.set_obstacle_track_offset(2 + t)
            r = pl.audited_tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"], margin, horizon, prev=prev,
                                tracked=True, late=late, early=early)
            pl.stop()
            a = pl.evaluate_paths_slack(sc["obstacles"], margin, late, early)
            s = pl.select_clear_slack(sc["obstacles"], margin, horizon, early, late, prev=r["pick"], first=7, skip_trailing=True)
            u = pl.evaluate_paths_tracked(sc["obstacles"], margin)
            differs = differs or not np.array_equal(u["clearance"], a["clearance"])
            prev = s["pick"]
            f = lines[t].split()
            p = r["pick"]
            print(lines[t], "|", r, s)
            assert [int(v) for v in f[:5]] == [t, p, r["rule"], r["n_clear"], r["first_violation"]]
            _same_bits(np.array(f[5:7], dtype=float), [r["cost"], r["clearance"]], "cost, clearance")
            _same_bits(np.array(f[7:10], dtype=float), pl.last_next_pos, "set-point")
            _same_bits(np.array([f[10], f[17]], dtype=float), [a["clearance"][p], s["clearance"]], "clearances")
            assert [int(v) for v in f[11:17]] == [a["step"][p], a["obstacle_step"][p], a["obstacle"][p], a["first_violation"][p],
                                                  s["pick"], s["first_violation"]]
        assert differs       # the tracked sphere closes in on this arm: the slacked audit is not the unslacked one
    finally:
        pl.close()


def test_audited_tick_without_slack_is_todays_tick(pmaf, scenes, hip_lib):
    """audited_tick(late = 0, early = 0) makes today's calls: the same picks and set-points as without the parameters"""
    sc = build_scene(scenes, 5, 3, 70)
    runs = []
    for kw in ({}, dict(late=0, early=0)):
        pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
        try:
            pl.set_initial_position(sc["start"])
            pl.start()
            rec = []
            for t in range(3):
                r = pl.audited_tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"], 0.05, 50, **kw)
                rec.append((r["pick"], r["rule"], pl.last_next_pos.copy()))
            runs.append(rec)
        finally:
            pl.close()
    for (p0, r0, x0), (p1, r1, x1) in zip(*runs):
        assert (p0, r0) == (p1, r1)
        _same_bits(x1, x0, "set-point")
