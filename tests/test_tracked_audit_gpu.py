"""The audits against the obstacle tracks on the GPU (pmaf_evaluate_paths_tracked / pmaf_select_clear_tracked,
k_ft_select_audit and k_audit_track_ft of csrc/pmaf_k_auditft.hip) through the C-ABI against
tests/tracked_audit_reference.py at TOLERANCE 0: integers equal, doubles bit-equal. The reference is fed the handle's
own paths(), n_points and costs(), the live list and the tracks as they were uploaded, and takes its dot association
from pmaf_eval_order(), so the file passes unchanged under PMAF_VARIANT=rassoc. tests/test_tracked_audit.py validates
the reference on the CPU and shows that the shapes are sensitive to every rule of the contract.

Shapes: N = 5 and 16 agents, P = 1 and 2, M = 1, 3, 59, 60 field obstacles (60 is the most a tracked handle can have),
cap 9 and 70, the PLAIN and the general step. The tracks are tests/field_track_reference.tracks_for's, built from the
handle's own untracked path of agent 0: obstacle 0 travels 0.25 m beside that path, obstacle M-1 below it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conftest
import field_track_reference as fref
import select_clear_reference as sref
import tracked_audit_reference as ref

pytestmark = pytest.mark.gpu

ROOT = conftest.ROOT
INT32_MAX = 2 ** 31 - 1
INT_KEYS = ("pick", "rule", "n_clear", "first_violation")
DBL_KEYS = ("cost", "clearance")
ERR_INVALID, ERR_STATE = -1, -3


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("PMAF_SUM", "PMAF_FORCE_GENERIC", "PMAF_PLAIN_STEP", "PMAF_MW", "PMAF_W64_SLICE"):
        monkeypatch.delenv(k, raising=False)


def _same_bits(got, want, what):
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float64).reshape(-1))
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float64).reshape(-1))
    assert got.shape == want.shape, what
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), "%s: %d of %d values differ, first at %s: %r != %r" % (
        what, (~ok).sum(), ok.size, np.argwhere(~ok)[0], got[~ok][0], want[~ok][0])


def build_scene(scenes, N, M, cap, general=False, scene_id=0):
    """tests/sentinel_track_reference.build_scene with the number of agents free"""
    sc = scenes.synthetic_scene(N, cap - 1, M, config_id=11, scene_id=scene_id, dynamic=False)
    sc["k_attr"] = np.linspace(3.0, 5.0, N)
    sc["k_repel"] = np.linspace(0.06, 0.1, N)
    if general:
        sc["agent_mass"] = 1.25
        sc["k_attr"][2] = 0.0
    at = sc["start"] + np.array([0.05, 0.3 + 0.02 * scene_id, 0.02])
    sc["obstacles"][-1] = [at[0], at[1], at[2], 0.3, 0.6, -0.2, 0.1]
    return sc


class Case:
    """a handle behind one untracked rollout and pmaf_evaluate, its tables as the references take them, the tracks built
    from its paths, and a live list: the field obstacles moved on and drifting, radii that are not the creation list's,
    the trailing obstacle -- a small sphere at rest -- ON agent 1's path, half way"""

    def __init__(self, pmaf, scenes, hip_lib, P, N, M, cap, general=False):
        self.scs = [build_scene(scenes, N, M, cap, general, p) for p in range(P)]
        self.sc = self.scs[0]
        starts = np.stack([s["start"] for s in self.scs])
        self.pl = pmaf.PmafPlanner(self.scs if P > 1 else self.sc, device=0, mgr_init_pos=starts)
        self.P, self.N, self.M, self.cap = P, N, M, cap
        self.order = hip_lib.pmaf_eval_order()
        self.pl.set_initial_position(starts)
        self.pl.rollout()
        self.pl.evaluate(self.sc["cost_gains"], self.sc["ws_limits"])
        self.refresh()
        self.tracks = [fref.tracks_for(sc, np.asarray(self.paths[p][0]), int(self.n[p][0])) for p, sc in enumerate(self.scs)]
        live = []
        for p, sc in enumerate(self.scs):
            o = np.array(sc["obstacles"], dtype=np.float64, copy=True)
            o[:M, 0:3] += 0.01
            o[:M, 3:6] += 0.02 * np.cos(np.arange(M)[:, None] + np.arange(3)[None, :])
            o[:M, 6] *= 1.1
            k = int(self.n[p][1]) // 2
            o[M] = list(self.paths[p][1][k]) + [0.0, 0.0, 0.0, 0.02]
            live.append(o)
        self.live = np.stack(live)
        self.attached = [None] * P     # what the handle has attached, as the reference takes it
        self.offset = [0] * P
        self._audited = {}             # the reference's window audits against self.live, computed once each

    def refresh(self):
        pl = self.pl
        paths, n = pl.paths()
        self.paths = np.asarray(paths).reshape(pl.P, pl.N, pl.cap, 3).tolist()
        self.n = np.asarray(n).reshape(pl.P, pl.N).tolist()
        self.costs = np.asarray(pl.costs()).reshape(pl.P, pl.N).tolist()

    def attach(self, tracks, offset=None):
        """tracks: a list over the populations of [L][M][6] or None"""
        self.pl.set_obstacle_tracks(tracks[0] if self.P == 1 else tracks)
        self.attached = [None if t is None else np.asarray(t).tolist() for t in tracks]
        self.offset = [0] * self.P
        self._audited = {}
        if offset is not None:
            self.set_offset(offset)

    def set_offset(self, offset):
        self.pl.set_obstacle_track_offset(offset)
        self.offset = list(offset)

    def close(self):
        self.pl.close()

    def _first(self, first):
        """(the call's argument, the offsets the reference uses)"""
        if first is None:
            return None, self.offset
        f = np.broadcast_to(np.asarray(first, dtype=np.int64), (self.P,)).tolist()
        return np.asarray(f, dtype=np.int32), f

    def check_select(self, margin, horizon, first=None, skip=False, prev=None, live=None, what=""):
        """one pmaf_select_clear_tracked call (adopt = 0) against the reference; returns the call's dict as arrays [P]"""
        live = self.live if live is None else live
        arg, f = self._first(first)
        got = self.pl.select_clear_tracked(live, margin, horizon, prev=prev, first=arg, skip_trailing=skip)
        got = {k: np.asarray(v).reshape(self.P) for k, v in got.items()}
        pv = None if prev is None else np.broadcast_to(np.asarray(prev), (self.P,)).tolist()
        audited = None
        if live is self.live:
            key = (margin, horizon, tuple(f), skip)
            if key not in self._audited:
                self._audited[key] = ref.window_audit(self.paths, self.n, live.tolist(), self.attached, f, self.sc["dt"],
                                                      self.sc["radius"], margin, horizon, skip, self.order)
            audited = self._audited[key]
        want = ref.select_clear(self.paths, self.n, live.tolist(), self.attached, f, self.costs, self.sc["dt"],
                                self.sc["radius"], margin, horizon, skip, self.order, pv, audited)
        tag = "%s select margin %r horizon %r first %r skip %r prev %r" % (what, margin, horizon, first, skip, prev)
        print(tag, "got", {k: v.tolist() for k, v in got.items()})
        for k in INT_KEYS:
            np.testing.assert_array_equal(got[k], np.asarray(want[k]), err_msg=k + " " + tag)
        for k in DBL_KEYS:
            _same_bits(got[k], want[k], k + " " + tag)
        return got

    def check_audit(self, margin, first=None, live=None, what=""):
        """one pmaf_evaluate_paths_tracked call against the reference; returns the call's dict as arrays [P][N]..."""
        live = self.live if live is None else live
        arg, f = self._first(first)
        got = self.pl.evaluate_paths_tracked(live, margin, per_obstacle=True, first=arg)
        got = {k: np.asarray(v).reshape((self.P, self.N) + ((self.M + 1,) if k == "per_obstacle" else ())) for k, v in got.items()}
        want = ref.audit(self.paths, self.n, live.tolist(), self.attached, f, self.sc["dt"], self.sc["radius"], margin, self.order)
        tag = "%s audit margin %r first %r" % (what, margin, first)
        print(tag, "clearance", got["clearance"].tolist(), "fv", got["first_violation"].tolist())
        for k in ("step", "obstacle", "first_violation"):
            np.testing.assert_array_equal(got[k], np.asarray(want[k]), err_msg=k + " " + tag)
        _same_bits(got["clearance"], want["clearance"], "clearance " + tag)
        _same_bits(got["per_obstacle"], want["per_obstacle"], "per_obstacle " + tag)
        return got


# (P, N, M, cap, general step)
SHAPES = [(1, 5, 1, 9, False), (1, 5, 3, 70, False), (2, 5, 3, 70, True), (1, 16, 59, 70, False), (2, 16, 60, 9, False),
          (1, 5, 60, 70, True)]
_ids = lambda s: "P%d-N%d-M%d-cap%d%s" % (s[0], s[1], s[2], s[3], "-general" if s[4] else "")


def _tracks(c, name):
    return [c.tracks[p][name] for p in range(c.P)]


# ---- 1. fails without the feature ---------------------------------------------------------------------------------------
def _far_list(c):
    """the case's live list with field obstacle 0 small, at rest and far away, and the trailing obstacle out of the way"""
    live = c.live.copy()
    live[:, 0] = [50.0, 50.0, 50.0, 0.0, 0.0, 0.0, 0.01]
    live[:, -1] = [100.0, 100.0, 100.0, 0.0, 0.0, 0.0, 0.02]
    return live


@pytest.mark.parametrize("shape", [(1, 5, 3, 70, False), (2, 16, 59, 70, False)], ids=_ids)
def test_the_selection_sees_where_the_track_puts_the_obstacle(pmaf, scenes, hip_lib, shape):
    """Obstacle 0 rests far away in the live list; its track passes through the cheapest clear agent's path point
    x_{k*} at point k*. pmaf_select_clear calls that agent clear, pmaf_select_clear_tracked does not. The mirror: the
    list's line cuts the path at k*, the track stays away: rejected by the untracked call, clear for the tracked one."""
    P, N, M, cap, general = shape
    c = Case(pmaf, scenes, hip_lib, P, N, M, cap, general)
    try:
        pl, dt = c.pl, c.sc["dt"]
        far = _far_list(c)
        horizon = cap
        plain = pl.select_clear(far, 0.0, horizon)
        plain = {k: np.asarray(v).reshape(P) for k, v in plain.items()}
        want = sref.select_clear(c.paths, c.n, far.tolist(), c.costs, dt, c.sc["radius"], 0.0, horizon, c.order)
        for k in INT_KEYS:
            np.testing.assert_array_equal(plain[k], np.asarray(want[k]), err_msg=k)
        for k in DBL_KEYS:
            _same_bits(plain[k], want[k], k)
        assert (plain["rule"] == 1).all()
        star = plain["pick"].tolist()
        w = [min(c.n[p][star[p]], horizon) for p in range(P)]
        assert plain["first_violation"].tolist() == w and min(w) >= 4     # the agent is clear in the untracked call
        kstar = [w[p] // 2 for p in range(P)]
        # the tracks: everybody on the far list's lines but obstacle 0, which is at x_{k*} at point k* only
        tracks = []
        for p in range(P):
            t = fref.straight_lines(far[p], dt, cap)
            t[kstar[p], 0, 0:3] = c.paths[p][star[p]][kstar[p]]
            tracks.append(t)
        c.attach(tracks)
        audit = c.check_audit(0.0, live=far, what="through the path")
        got = c.check_select(0.0, horizon, live=far, what="through the path")
        again = c.check_select(0.0, horizon, live=far, prev=star, what="through the path, prev = the blocked agent")
        for p in range(P):
            assert audit["first_violation"][p][star[p]] == kstar[p]
            assert audit["obstacle"][p][star[p]] == 0 and audit["step"][p][star[p]] == kstar[p]
            for r in (got, again):
                assert not (r["rule"][p] in (0, 1) and r["pick"][p] == star[p])
        # the untracked call on the same handle still calls the agent clear: it does not see the tracks
        still = pl.select_clear(far, 0.0, horizon)
        np.testing.assert_array_equal(np.asarray(still["pick"]).reshape(P), plain["pick"])
        # the mirror: the list's line reaches x_{k*} at step k*; the track rests far away
        cut = far.copy()
        for p in range(P):
            x = np.asarray(c.paths[p][star[p]][kstar[p]])
            v = np.array([0.3, -0.2, 0.1])
            cut[p, 0] = list(x - kstar[p] * (v * dt)) + list(v) + [0.01]
        c.attach([fref.straight_lines(far[p], dt, cap) for p in range(P)])
        un = pl.evaluate_paths(cut, 0.0)
        un_fv = np.asarray(un["first_violation"]).reshape(P, N)
        audit = c.check_audit(0.0, live=cut, what="mirror")
        got = c.check_select(0.0, horizon, live=cut, prev=star, what="mirror")
        for p in range(P):
            assert un_fv[p][star[p]] <= kstar[p] < w[p]                    # rejected by the untracked audit
            assert audit["first_violation"][p][star[p]] == c.n[p][star[p]]
            assert got["rule"][p] == 0 and got["pick"][p] == star[p]       # clear, and kept
    finally:
        c.close()


# ---- 2. no tracks attached; one population at L = 0 ---------------------------------------------------------------------
def _device_against_device(c, live, margin, horizon, pops, prev=None):
    """the tracked calls against the untracked ones on the same handle, populations `pops`"""
    pl = c.pl
    a = pl.select_clear(live, margin, horizon, prev=prev)
    b = pl.select_clear_tracked(live, margin, horizon, prev=prev)
    for k in INT_KEYS + DBL_KEYS:
        _same_bits(np.asarray(b[k], dtype=np.float64).reshape(c.P)[pops], np.asarray(a[k], dtype=np.float64).reshape(c.P)[pops], k)
    a = pl.evaluate_paths(live, margin, per_obstacle=True)
    b = pl.evaluate_paths_tracked(live, margin, per_obstacle=True)
    for k in a:
        shape = (c.P, c.N) + ((c.M + 1,) if k == "per_obstacle" else ())
        _same_bits(np.asarray(b[k], dtype=np.float64).reshape(shape)[pops], np.asarray(a[k], dtype=np.float64).reshape(shape)[pops], k)


@pytest.mark.parametrize("shape", [(1, 5, 3, 9, False), (2, 16, 59, 70, False), (2, 5, 66, 9, False)], ids=_ids)
def test_without_tracks_the_untracked_result(pmaf, scenes, hip_lib, shape):
    """first = NULL on a handle without tracks (also one of more than 64 obstacles, which can have none)"""
    c = Case(pmaf, scenes, hip_lib, *shape)
    try:
        for margin, horizon in ((0.0, c.cap), (0.05, 3), (3.0, c.cap + 5)):
            _device_against_device(c, c.live, margin, horizon, list(range(c.P)), prev=[1] * c.P)
        c.check_select(0.0, c.cap, prev=1)
        c.check_audit(0.0)
    finally:
        c.close()


def test_one_population_without_tracks(pmaf, scenes, hip_lib):
    c = Case(pmaf, scenes, hip_lib, 2, 5, 3, 70)
    try:
        for given, untracked_pop in (([c.tracks[0]["Lcap"], None], 1), ([None, c.tracks[1]["short"]], 0)):
            c.attach(given, [1, 2])
            for margin, horizon in ((0.0, c.cap), (0.1, 7)):
                _device_against_device(c, c.live, margin, horizon, [untracked_pop])
                c.check_select(margin, horizon, prev=[0, 2])
            c.check_audit(0.0)
            c.check_select(0.0, c.cap, first=[3, 0], skip=True)
    finally:
        c.close()


# ---- 3. straight-line tracks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 1, 9, False), (2, 16, 60, 70, True)], ids=_ids)
def test_straight_line_tracks_give_the_untracked_bits(pmaf, scenes, hip_lib, shape):
    c = Case(pmaf, scenes, hip_lib, *shape)
    try:
        c.attach([fref.straight_lines(c.live[p], c.sc["dt"], c.cap + 5) for p in range(c.P)])
        for margin, horizon in ((0.0, c.cap), (0.05, 5), (3.0, c.cap + 5), (-0.5, 1)):
            _device_against_device(c, c.live, margin, horizon, list(range(c.P)), prev=[2] * c.P)
        c.check_select(0.0, c.cap)
        c.check_audit(0.0)
    finally:
        c.close()


# ---- 4. - 6., 8. lengths and offsets, horizons and windows, the rules, the audit ------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_lengths_offsets_windows_rules(pmaf, scenes, hip_lib, shape):
    c = Case(pmaf, scenes, hip_lib, *shape)
    P, cap = c.P, c.cap
    try:
        # track lengths 1, 2, cap, cap + 5 and one that ends mid-path (the held end); offsets 0, 1, L-1, L+3, INT32_MAX
        for name, first in (("L1", 0), ("L2", 1), ("Lcap", "L-1"), ("Lcap+5", 1), ("short", "L+3"), ("short", INT32_MAX),
                            ("Lcap", 0), ("short", 1)):
            t = _tracks(c, name)
            f = [fref.resolve_first(first, len(t[p])) for p in range(P)]
            c.attach(t)
            c.check_select(0.0, cap + 5, first=f, prev=1, what=name)
            c.check_audit(0.0, first=f, what=name)
        # first = NULL after pmaf_set_obstacle_track_offset; an explicit offset then overrides the handle's
        c.attach(_tracks(c, "short"), [2] * P)
        a = c.check_select(0.0, cap, what="handle offset")
        b = c.check_select(0.0, cap, first=2, what="the same offset given")
        for k in INT_KEYS + DBL_KEYS:
            _same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), k)
        c.check_audit(0.02, what="handle offset")
        c.check_select(0.0, cap, first=0, what="explicit 0 over the handle's 2")
        _, first_now = c.pl.get_obstacle_tracks()
        assert list(first_now) == [2] * P          # the call's offsets did not become the handle's
        # horizons: 1; 3 (fewer points than waves); 5 and 7 (the window ends inside a quarter); cap; above cap --
        # with and without the trailing obstacle, which sits on agent 1's path
        c.attach(_tracks(c, "Lcap+5"), [1] * P)
        for horizon in (1, 3, 5, 7, cap, cap + 6):
            for skip in (False, True):
                c.check_select(0.0, horizon, skip=skip, prev=[1] * P, what="horizon")
        w = c.check_select(0.0, cap, skip=False)
        s = c.check_select(0.0, cap, skip=True)
        assert (s["n_clear"] >= w["n_clear"]).all()
        # the rules: in between; nobody clear (2, the fallback); everybody clear (1, the cheapest; 0, the previous pick kept)
        for margin in (0.05, 0.15):
            for prev in (None, [(p + 2) % c.N for p in range(P)], -1):
                c.check_select(margin, cap, prev=prev, what="rules")
        r = c.check_select(3.0, cap)
        assert (r["rule"] == 2).all() and (r["n_clear"] == 0).all()
        r = c.check_select(-0.5, cap)
        assert (r["rule"] == 1).all() and (r["n_clear"] == c.N).all()
        r = c.check_select(-0.5, cap, prev=r["pick"].tolist())       # the cheapest clear agent as the previous pick: kept
        assert (r["rule"] == 0).all()
        c.check_audit(0.15, first=3)
    finally:
        c.close()


@pytest.mark.parametrize("horizon", [1, 2, 3, 5])
def test_windows_shorter_than_two_points_per_wave(pmaf, scenes, hip_lib, horizon):
    """the audit splits the window of w = min(n, horizon) points over four waves in quarters of ceil(w / 4): w = 1, 2, 3
    leave waves without a step, w = 5 gives quarters of 2, 2, 1, 0 -- at P = 2, N = 5, M = 3, cap = 9, on tracks read
    from their start, from the middle, and from an offset at or past the last point (every step holds it); and on the
    same handle without tracks, where the tracked call runs the untracked kernel"""
    c = Case(pmaf, scenes, hip_lib, 2, 5, 3, 9)
    try:
        assert all(n >= 5 for row in c.n for n in row)      # w = horizon for every agent
        for margin in (0.0, 0.1):
            c.check_select(margin, horizon, prev=[1, 3], what="no tracks")
        for name, first in (("Lcap", 0), ("short", 1), ("Lcap", "L-1"), ("short", "L+3"), ("L2", INT32_MAX)):
            t = _tracks(c, name)
            c.attach(t)
            f = [fref.resolve_first(first, len(t[p])) for p in range(c.P)]
            for margin in (0.0, 0.1):
                for skip in (False, True):
                    got = c.check_select(margin, horizon, first=f, skip=skip, prev=[1, 3], what=name)
                    assert (got["first_violation"] <= horizon).all()
    finally:
        c.close()


def test_a_tie_between_a_tracked_and_the_trailing_obstacle_goes_to_the_smaller_index(pmaf, scenes, hip_lib):
    c = Case(pmaf, scenes, hip_lib, 1, 5, 3, 70)
    try:
        k = c.n[0][0] // 2
        x = c.paths[0][0][k]
        live = c.live.copy()
        live[0, -1] = list(x) + [0.0, 0.0, 0.0, 0.03]
        live[0, 0, 6] = 0.03
        t = np.array(c.tracks[0]["Lcap"], copy=True)
        t[:, 0, 0:3] = x                             # obstacle 0 rests where the trailing obstacle rests
        c.attach([t])
        got = c.check_audit(0.0, live=live)
        assert got["obstacle"][0][0] == 0 and got["step"][0][0] == k
        _same_bits(got["per_obstacle"][0][0][0], got["per_obstacle"][0][0][3], "the two columns tie")
        assert got["clearance"][0][0] == -(c.sc["radius"] + 0.03)
        c.check_select(0.0, c.cap, live=live)
    finally:
        c.close()


def test_optional_outputs_may_be_null(pmaf, scenes, hip_lib):
    c = Case(pmaf, scenes, hip_lib, 1, 5, 3, 9)
    try:
        c.attach(_tracks(c, "L2"))
        L, h = hip_lib, c.pl._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        obs = np.ascontiguousarray(c.live, dtype=np.float64)
        full = c.check_select(0.0, 9, first=1)
        pick = np.full(1, -7, dtype=np.int32)
        assert L.pmaf_select_clear_tracked(h, obs.ctypes.data_as(dp), None, 0.0, 9, 0, None, 0, pick.ctypes.data_as(ip), None,
                                           None, None, None, None) == 0
        f1 = np.array([1], dtype=np.int32)
        assert L.pmaf_select_clear_tracked(h, obs.ctypes.data_as(dp), f1.ctypes.data_as(ip), 0.0, 9, 0, None, 0,
                                           pick.ctypes.data_as(ip), None, None, None, None, None) == 0
        assert pick[0] == full["pick"][0]
        assert L.pmaf_select_clear_tracked(h, obs.ctypes.data_as(dp), None, 0.0, 9, 0, None, 0, None, None, None, None, None, None) == ERR_INVALID
        clr = np.zeros(5)
        assert L.pmaf_evaluate_paths_tracked(h, obs.ctypes.data_as(dp), f1.ctypes.data_as(ip), 0.0, clr.ctypes.data_as(dp), None,
                                             None, None, None) == 0
        _same_bits(clr, c.check_audit(0.0, first=1)["clearance"], "clearance alone")
    finally:
        c.close()


# ---- 7. state --------------------------------------------------------------------------------------------------------------
def _state(pl):
    t, i = pl.best()
    pos, vel, force = pl.real_state()
    known, rot = pl.real_known()
    return (np.asarray(t).copy(), np.asarray(i).copy(), np.asarray(known).copy(),
            [np.asarray(a).copy() for a in (pos, vel, force, rot)])


def test_adoption_steers_the_real_step(pmaf, scenes, hip_lib):
    """adopt = 1: pmaf_get_best names the pick, and the next pmaf_move_real is the one of a handle that selected with
    adopt = 0 and adopted the pick through pmaf_adopt_best"""
    cs = [Case(pmaf, scenes, hip_lib, 2, 5, 3, 70, True) for _ in range(2)]
    try:
        picks = []
        for i, c in enumerate(cs):
            c.attach(_tracks(c, "Lcap"), [1, 2])
            before = np.asarray(c.pl.best()[1]).copy()
            r = c.pl.select_clear_tracked(c.live, 0.0, c.cap, prev=[1, 1], adopt=(i == 0))
            pick = np.asarray(r["pick"]).reshape(2)
            picks.append(pick)
            if i == 0:
                np.testing.assert_array_equal(c.pl.best()[1], pick + 1)
            else:
                np.testing.assert_array_equal(c.pl.best()[1], before)
                c.pl.adopt_best(pick)
            c.pl.move_real(c.live, c.sc["dt"], 1, pick)
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
    """six closed-loop ticks with the offset one further in front of each, with and without tracked audits (adopt = 0, own
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
                    r = pl.select_clear_tracked(live, 0.05, 50 if t % 2 else 1000, prev=int(b), first=None if t % 3 else t + 4)
                    assert 0 <= r["pick"] < pl.N
                    pl.evaluate_paths_tracked(live, 0.05, first=t)
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


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------
def test_errors_and_a_shorter_upload(pmaf, scenes, hip_lib):
    c = Case(pmaf, scenes, hip_lib, 2, 5, 3, 70)
    try:
        pl = c.pl
        for call in (lambda **kw: pl.select_clear_tracked(c.live, kw.get("margin", 0.0), 9, first=kw.get("first")),
                     lambda **kw: pl.evaluate_paths_tracked(c.live, kw.get("margin", 0.0), first=kw.get("first"))):
            with pytest.raises(pmaf.PmafError) as e:        # an offset on a handle without tracks
                call(first=[0, 0])
            assert e.value.code == ERR_STATE, str(e.value)
            with pytest.raises(pmaf.PmafError) as e:        # ... a negative one is refused first
                call(first=[0, -1])
            assert e.value.code == ERR_INVALID, str(e.value)
            call()                                          # first = NULL is the untracked call
        c.attach(_tracks(c, "Lcap+5"), [1, 1])
        for call in (lambda **kw: pl.select_clear_tracked(c.live, kw.get("margin", 0.0), 9, first=kw.get("first")),
                     lambda **kw: pl.evaluate_paths_tracked(c.live, kw.get("margin", 0.0), first=kw.get("first"))):
            with pytest.raises(pmaf.PmafError) as e:
                call(first=[3, -1])
            assert e.value.code == ERR_INVALID and "first" in str(e.value), str(e.value)
            with pytest.raises(pmaf.PmafError) as e:
                call(margin=float("nan"))
            assert e.value.code == ERR_INVALID and "range" in str(e.value), str(e.value)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_tracked(c.live, 0.0, 0)
        assert e.value.code == ERR_INVALID and "horizon" in str(e.value)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_tracked(c.live, 0.0, 9, prev=[5, 0])
        assert e.value.code == ERR_INVALID and "prev_idx" in str(e.value)
        # a shorter upload after the longer one: the audit holds the SHORT tracks' last point, no stale point of the long
        c.check_audit(0.0, first=[0, 2], what="long")
        short = [np.array(c.tracks[p]["L2"], copy=True) + 0.004 for p in range(2)]
        c.attach(short)
        c.check_audit(0.0, what="short after long")
        c.check_select(0.0, c.cap, first=[1, 0], what="short after long")
        c.attach([None, None])                              # detached: an offset is refused again, NULL is untracked
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_tracked(c.live, 0.0, 9, first=[0, 0])
        assert e.value.code == ERR_STATE
        _device_against_device(c, c.live, 0.0, c.cap, [0, 1])
    finally:
        c.close()


def test_refused_after_an_abandoned_tick(pmaf, scenes, hip_lib, monkeypatch):
    """tests/test_select_clear_gpu.py's abandoned tick: pmaf_select_clear_tracked refuses the handle until pmaf_stop"""
    monkeypatch.setenv("PMAF_TICK_TIMEOUT_S", "0.002")
    sc = scenes.synthetic_scene(512, 6000, 128, 3, 1)       # ~15 ms of rollout per tick
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        pl.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
        pl.stop()
        pl.debug_withhold_mailbox(True)
        with pytest.raises(pmaf.PmafError) as e:
            pl.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
        assert e.value.code == -2 and "time limit" in str(e.value), str(e.value)
        pl.debug_withhold_mailbox(False)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_tracked(sc["obstacles"], 0.05, 5)
        assert e.value.code == ERR_STATE, str(e.value)
        pl.stop()
        r = pl.select_clear_tracked(sc["obstacles"], 0.05, 5)
        assert 0 <= r["pick"] < 512
    finally:
        pl.close()


# ---- 10. the facade ----------------------------------------------------------------------------------------------------------
def test_facade_tracked_audit_equals_the_c_abi_sequence(pmaf, scenes, tmp_path, hip_lib):
    """tests/cpp/facade_tracked_audit.cpp runs CfManager::planTickAudited(tracked = true) over 5 ticks with
    advanceObstacleTracks in between, then evaluatePathsTracked and selectClearTracked; every figure it prints equals the
    same calls made through the binding"""
    N, cap, ticks, L, margin, horizon = 12, 101, 5, 40, 0.05, 60
    sc = scenes.static1_scene(N, cap - 1)
    rvf = tmp_path / "rv.bin"
    np.ascontiguousarray(sc["random_vecs"]).tofile(rvf)
    exe = conftest.exe(os.path.join(ROOT, "tests", "cpp", "facade_tracked_audit"))
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    out = subprocess.run([exe, str(N), str(cap), str(ticks), str(rvf), str(L), repr(margin), str(horizon)], capture_output=True,
                         check=True, env=conftest.binary_env(pmaf)).stdout.decode()
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
            r = pl.audited_tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"], margin, horizon, prev=prev, tracked=True)
            pl.stop()
            a = pl.evaluate_paths_tracked(sc["obstacles"], margin)
            b = pl.evaluate_paths_tracked(sc["obstacles"], margin, first=7)
            s = pl.select_clear_tracked(sc["obstacles"], margin, horizon, prev=r["pick"], first=7, skip_trailing=True)
            u = pl.evaluate_paths(sc["obstacles"], margin)
            differs = differs or not np.array_equal(u["clearance"], a["clearance"])
            prev = s["pick"]
            f = lines[t].split()
            p = r["pick"]
            print(lines[t], "|", r, s)
            assert [int(v) for v in f[:5]] == [t, p, r["rule"], r["n_clear"], r["first_violation"]]
            _same_bits(np.array(f[5:7], dtype=float), [r["cost"], r["clearance"]], "cost, clearance")
            _same_bits(np.array(f[7:10], dtype=float), pl.last_next_pos, "set-point")
            _same_bits(np.array([f[10], f[13], f[17]], dtype=float), [a["clearance"][p], b["clearance"][p], s["clearance"]], "clearances")
            assert [int(f[11]), int(f[12]), int(f[14]), int(f[15]), int(f[16])] == [
                a["step"][p], a["first_violation"][p], b["obstacle"][p], s["pick"], s["first_violation"]]
        assert differs       # the tracked sphere is near this arm: the tracked audit is not the untracked one
    finally:
        pl.close()
