"""The joint selection on coupled handles on the GPU (pmaf_cross_audit_attached / pmaf_select_pair_clear_tracked;
k_cross_audit_attached of csrc/pmaf_k_xattach.hip and k_ft_masked_audit of csrc/pmaf_k_auditft.hip) through the C-ABI, at
tolerance 0 against tests/attached_audit_reference.py on the handle's own paths, costs and composed tracks.
tests/test_attached_audit.py validates the reference on the CPU, shows which rule each case is sensitive to and asserts
the pre-conditions of the behavioural cases below on the same scenes. The references take the evaluation order from
pmaf_eval_order(), so the file passes unchanged under PMAF_VARIANT=rassoc.

Shapes follow the kernel's own constants (csrc/pmaf_cross_audit.hpp): T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK -- N = 5
and T + 1 (a ragged second tile on both axes), capacities 9 (below one chunk) and 70 (four chunks and a ragged fifth)."""
import ctypes as C

import numpy as np
import pytest

import attached_audit_cases as cases
import attached_audit_reference as ref
from test_attached_audit import BEHAVIOUR, BEHAVIOUR_SHAPES, behaviour_step, tie_separation
from test_cross_audit_gpu import CH, T
from test_select_clear_gpu import _same_bits, _same_state, _state

pytestmark = pytest.mark.gpu

INT_KEYS = ("pair", "rule", "n_feasible", "n_clear", "first_violation", "steps")
DBL_KEYS = ("cost", "clearance", "obstacle_clearance", "worst_excess")
ERR_INVALID, ERR_STATE = -1, -3


def test_the_shapes_follow_the_kernel_constants():
    assert cases.T == T and cases.SHAPES["P2-N33-M3-cap70-ragged"]["N"] == T + 1
    assert 9 < CH and 70 > 4 * CH and 70 % CH != 0


def _compare(got, want, tag):
    print(tag, "got", got)
    for k in INT_KEYS:
        assert got[k] == want[k], "%s: %s %r != %r" % (tag, k, got[k], want[k])
    for k in DBL_KEYS:
        _same_bits(got[k], want[k], k + " " + tag)


def _matrices(got, want, tag):
    _same_bits(got[0], want[0], tag + " clearance")
    np.testing.assert_array_equal(np.asarray(got[1]), np.asarray(want[1]), err_msg=tag + " step")
    np.testing.assert_array_equal(np.asarray(got[2]), np.asarray(want[2]), err_msg=tag + " sphere")


def _planner(pmaf, scs):
    starts = np.stack([s["start"] for s in scs])
    pl = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    pl.set_initial_position(starts)
    return pl


def _couple(pl, cpl):
    if cpl is None:
        pl.couple_obstacle_tracks(None)
    else:
        pl.couple_obstacle_tracks(cpl["src"], cpl["scale"], cpl["anchor"], cpl["shift"])


def _coupled_state(pmaf, scenes, shape, kind, ticks=2):
    """a handle of the shape with the kind's coupling after `ticks` ticks: the paths of the last launch, which followed
    tracks composed from the selection in front of it, scored"""
    scs = cases.build_scenes(scenes, shape)
    pl = _planner(pmaf, scs)
    cpl = cases.coupling(shape, kind, scs)
    _couple(pl, cpl)
    obs0 = np.stack([s["obstacles"] for s in scs])
    pl.start()
    pl.stop()
    for _ in range(ticks):
        pl.tick(obs0, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
    pl.stop()
    pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
    return pl, scs, cpl


class Shared:
    """the reference's audits and matrices of one handle state, computed once per key and never modified"""

    def __init__(self, pl, scs, cpl, live, order):
        self.pl, self.cpl, self.order = pl, cpl, order
        self.dt, self.rad = scs[0]["dt"], scs[0]["radius"]
        self.live = np.asarray(live).tolist()
        paths, n = pl.paths()
        self.paths = np.asarray(paths).reshape(pl.P, pl.N, pl.cap, 3).tolist()
        self.n = np.asarray(n).reshape(pl.P, pl.N).tolist()
        self.costs = np.asarray(pl.costs()).reshape(pl.P, pl.N).tolist()
        used, first = pl.get_obstacle_tracks()
        self.tracks = [np.asarray(t).tolist() if len(t) else None for t in used]
        self.tracked = any(t is not None for t in self.tracks)
        self.aud, self.mat = {}, {}

    def sides(self, a, b, om, horizon, skip, sep, first):
        ka = (a, b, om, horizon, skip, None if first is None else tuple(first))
        km = (a, b, horizon, sep)
        if ka not in self.aud:
            self.aud[ka] = ref.obstacle_side(self.paths, self.n, self.live, self.tracks, first, self.cpl, a, b, self.dt,
                                             self.rad, om, horizon, skip, self.order)
        if km not in self.mat:
            self.mat[km] = ref.pair_side(self.paths[a], self.n[a], self.paths[b], self.n[b], self.cpl, a, b, self.live,
                                         self.rad, horizon, sep, self.order)
        return self.aud[ka], self.mat[km]

    def want(self, a, b, c, sep, first=None):
        aud, mat = self.sides(a, b, c["obstacle_margin"], c["horizon"], c["skip_trailing"], sep, first)
        return ref.select_pair_clear_tracked(self.paths, self.n, self.live, self.tracks, first, self.cpl, self.costs, self.dt,
                                             self.rad, a, b, c["obstacle_margin"], c["horizon"], c["skip_trailing"], sep,
                                             c["pair_margin"], c["prev_pair"], self.order, aud, mat)

    def call(self, a, b, c, sep, first=None, adopt=False):
        return self.pl.select_pair_clear_tracked(a, b, self.live, c["obstacle_margin"], c["horizon"], sep, c["pair_margin"],
                                                 skip_trailing=c["skip_trailing"], prev_pair=c["prev_pair"], adopt=adopt,
                                                 first=first)

    def check(self, a, b, c, sep=cases.SEP, first=None, tag=""):
        got = self.call(a, b, c, sep, first)
        _compare(got, self.want(a, b, c, sep, first), "%s %r first %r" % (tag, c, first))
        return got

    def whole(self, a, b, sep=cases.SEP):
        """the attached audit on the whole paths, device and reference"""
        got = self.pl.cross_audit_attached(a, b, self.live, sep, step=True, sphere=True)
        want = ref.cross_audit_attached(self.paths[a], self.n[a], self.paths[b], self.n[b], self.cpl, a, b, self.live,
                                        self.rad, sep, self.order)
        return got, want


def _call(horizon, om, pm, skip=0, prev=None):
    return dict(horizon=horizon, obstacle_margin=om, pair_margin=pm, skip_trailing=skip, prev_pair=prev)


def _median(values):
    v = sorted(x for x in values if x == x and abs(x) != float("inf"))
    return v[len(v) // 2] if v else 0.0


CASES = [(s, k) for s in cases.SHAPES for k in cases.kinds(s) if cases.SHAPES[s]["N"] == 5] + \
        [("P2-N33-M3-cap70-ragged", "none"), ("P2-N33-M3-cap70-ragged", "three")]
_SEEN = {}


def _run_case(pmaf, scenes, hip_lib, shape, kind):
    """one (shape, attachment kind): the attached matrices on the whole paths and the joint selection over horizons,
    margins (the extremes, and values that cut through the REFERENCE's own clearances), both skip settings, previous
    pairs and offsets; returns the (rule, n_feasible regime) pairs seen. Run once per case and session."""
    if (shape, kind) in _SEEN:
        return _SEEN[(shape, kind)]
    s = cases.SHAPES[shape]
    pl, scs, cpl = _coupled_state(pmaf, scenes, shape, kind)
    seen = set()
    try:
        N, cap = s["N"], s["cap"]
        live = cases.live_list(scenes, scs)
        sh = Shared(pl, scs, cpl, live, hip_lib.pmaf_eval_order())
        assert sh.tracked == (kind != "none")
        if s["ragged"]:
            assert len(set(sh.n[1])) > 1, "the ragged case is meant to have paths of different lengths"
        seps = (cases.SEP, tie_separation(scs, sh.live)) if kind == "tie" else (cases.SEP,)
        for sep in seps:
            got, want = sh.whole(0, 1, sep)
            _matrices(got, want, "%s %s sep %r" % (shape, kind, sep))
            print("sphere codes that win:", sorted(set(np.asarray(want[2]).reshape(-1).tolist())))
        if kind == "tie":      # the tie goes to the smallest term: the end effectors keep the pairs they decide
            assert 1 not in np.asarray(got[2]) and (np.asarray(got[2]) == 0).any()
        if kind == "none":     # device against device
            clr, st = pl.cross_audit(0, 1, cases.SEP, step=True)
            _same_bits(got[0], clr, "pmaf_cross_audit")
            np.testing.assert_array_equal(got[1], st)
            assert (np.asarray(got[2]) == np.where(st >= 0, 0, -1)).all()
        big = N > 5 or s["M"] > 3      # (the plain-Python reference of 1 089 pairs, or of 61 obstacles and 61 terms)
        horizons = (3, cap + 1) if big else (1, 3, cap // 2, cap + 1, cap + 6)
        k = 0
        for horizon in horizons:
            for skip in (0, 1):
                aud, mat = sh.sides(0, 1, -0.5, horizon, skip, cases.SEP, None)
                om_mid = _median(aud[0][0] + aud[0][1])
                pm_mid = _median([v for row in mat[0] for v in row])
                margins = [(-0.5, -0.5), (3.0, -0.5), (-0.5, 3.0), (om_mid, pm_mid), (-0.5, pm_mid), (om_mid, -0.5)]
                for om, pm in (margins[3:5] if big else margins):
                    for with_prev in (0, 1):
                        prev = ((3 * k) % N, (5 * k + 1) % N) if with_prev else None
                        first = [k % 3, (k + 1) % 4] + [0] * (pl.P - 2) if (sh.tracked and k % 2) else None
                        c = _call(horizon, om, pm, skip, prev)
                        r = sh.check(0, 1, c, first=first, tag="%s %s" % (shape, kind))
                        seen.add((r["rule"], 0 if r["n_feasible"] == 0 else (2 if r["n_feasible"] == N * N else 1)))
                        if kind == "none":      # device against device: the untracked joint call
                            u = pl.select_pair_clear(0, 1, live, om, horizon, cases.SEP, pm, skip_trailing=skip, prev_pair=prev)
                            _compare(r, u, "pmaf_select_pair_clear %r" % (c,))
                        k += 1
        if pl.P > 2 and not big:      # population offsets with a > b, and the third population as a member
            for a, b in ((1, 0), (2, 0), (1, 2)):
                got, want = sh.whole(a, b)
                _matrices(got, want, "%s %s pops %d %d" % (shape, kind, a, b))
                sh.check(a, b, _call(cap, 0.0, 0.0, 1, (1, 2)), tag="pops %d %d" % (a, b))
    finally:
        pl.close()
    _SEEN[(shape, kind)] = seen
    return seen


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: str(v))
def test_shapes_attachments_horizons_margins(pmaf, scenes, hip_lib, shape, kind):
    seen = _run_case(pmaf, scenes, hip_lib, shape, kind)
    print("(rule, n_feasible regime) seen:", sorted(seen))
    assert seen


def test_every_rule_and_every_n_feasible_regime_occurred(pmaf, scenes, hip_lib):
    seen = set()
    for shape, kind in CASES:
        seen |= _run_case(pmaf, scenes, hip_lib, shape, kind)
    print("(rule, n_feasible regime) over the whole parametrisation:", sorted(seen))
    assert {r for r, _ in seen} == {0, 1, 2}
    assert {g for _, g in seen} == {0, 1, 2}     # no pair feasible, some, all


# ---- the case that fails without the feature, and its mirror ----
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("shape", BEHAVIOUR_SHAPES)
def test_a_sphere_riding_on_the_other_member_rejects_the_pair(pmaf, scenes, hip_lib, shape, side):
    """After a rollout the untracked call picks (i*, j*). A column of A's list (side 0; of B's: side 1) is then attached
    with scale 1 and anchor x_i*(k) - y_j*(k): the sphere riding on j* sits on i*'s point at step k. Its live-list row
    is far away, so pmaf_select_pair_clear still returns (i*, j*); the new call does not, and equals the reference.
    (tests/test_attached_audit.py asserts the same on the oracle's rollouts of these scenes.)"""
    scs = cases.build_scenes(scenes, shape)
    pl = _planner(pmaf, scs)
    try:
        pl.rollout()
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        live = cases.live_list(scenes, scs)
        b, cap = BEHAVIOUR, pl.cap
        plain = pl.select_pair_clear(0, 1, live, b["obstacle_margin"], cap, cases.SEP, b["pair_margin"],
                                     skip_trailing=b["skip_trailing"])
        assert plain["rule"] in (0, 1) and plain["pair"][0] >= 0, plain
        paths, n = pl.paths()
        paths, n = np.asarray(paths).reshape(2, pl.N, cap, 3), np.asarray(n).reshape(2, pl.N)
        k = behaviour_step(n, plain["pair"], cap)
        cpl = cases.sphere_on_the_pair(2, pl.n_obs - 1, paths, n, plain["pair"], k, side)
        far = cases.far_rows(live, cpl)
        _couple(pl, cpl)
        again = pl.select_pair_clear(0, 1, far, b["obstacle_margin"], cap, cases.SEP, b["pair_margin"],
                                     skip_trailing=b["skip_trailing"])
        assert again["pair"] == plain["pair"] and again["rule"] == plain["rule"]
        sh = Shared(pl, scs, cpl, far, hip_lib.pmaf_eval_order())
        assert not sh.tracked      # (coupled, nothing composed yet: L = 0)
        got = sh.check(0, 1, _call(cap, b["obstacle_margin"], b["pair_margin"], b["skip_trailing"]), tag="behaviour")
        print("untracked", plain["pair"], "attached", got["pair"], "rule", got["rule"], "clearance", got["clearance"])
        assert got["pair"] != plain["pair"]
        clr, st, sp = pl.cross_audit_attached(0, 1, far, cases.SEP, step=True, sphere=True)
        i, j = plain["pair"]
        code = 1 if side == 0 else 1 + (pl.n_obs - 1)
        assert sp[i][j] == code and clr[i][j] < 0.0
        # uncoupled again: the untracked answer
        _couple(pl, None)
        _compare(pl.select_pair_clear_tracked(0, 1, far, b["obstacle_margin"], cap, cases.SEP, b["pair_margin"],
                                              skip_trailing=b["skip_trailing"]), again, "uncoupled")
    finally:
        pl.close()


def test_third_population_columns_stay_and_stale_tracks_do_not_violate(pmaf, scenes, hip_lib):
    """P = 3. Column 0 of arm 0's list rides on arm 1 (a term of the pair: left out of the obstacle side, although its
    stale track is put THROUGH arm 0's paths with uploaded tracks); column 2, put through the paths the same way, is not
    attached to the pair's populations and violates as pmaf_select_clear_tracked has it."""
    shape = "P3-N5-M3-cap70-ragged"
    scs = cases.build_scenes(scenes, shape)
    pl = _planner(pmaf, scs)
    try:
        pl.rollout()
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        live = cases.live_list(scenes, scs)
        cpl = cases.coupling(shape, "one", scs)
        # the coupling of populations 1 and 2 is empty: only arm 0 is coupled, and a coupled population cannot carry
        # uploaded tracks. So the stale track is what a launch composes: arm 0 rides column 0 on arm 1's selection. The
        # sphere is put through arm 0's paths by the anchor instead.
        paths, n = pl.paths()
        paths, n = np.asarray(paths).reshape(3, pl.N, pl.cap, 3), np.asarray(n).reshape(3, pl.N)
        best = [int(v) - 1 for v in pl.best()[1]]
        x0 = paths[0][best[0]][min(20, int(n[0][best[0]]) - 1)]
        for col in (0, 2):
            cpl["scale"][0][col] = 0.0
            cpl["anchor"][0][col] = x0      # at rest a few centimetres down arm 0's path: every path of arm 0 starts inside it
        cpl["shift"] = 0
        _couple(pl, cpl)
        obs0 = np.stack([s["obstacles"] for s in scs])
        pl.tick(obs0, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
        pl.stop()
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        sh = Shared(pl, scs, cpl, live, hip_lib.pmaf_eval_order())
        assert sh.tracks[0] is not None and sh.tracks[1] is None
        start0 = np.asarray(sh.paths[0][0][0])
        t0 = np.asarray(sh.tracks[0])
        near = [float(np.linalg.norm(t0[0, col, 0:3] - start0)) for col in (0, 2)]
        print("distance of the two composed spheres from arm 0's rollout start:", near)
        assert max(near) < 0.1
        # pair (0, 1): column 0 is the pair side's, column 2 still cuts every path of arm 0
        c = _call(pl.cap, 0.0, -0.5, 1)
        got = sh.check(0, 1, c, tag="pair 0 1")
        assert got["n_clear"][0] == 0
        # pair (0, 2): now column 2 is the pair side's and column 0 stays
        got = sh.check(0, 2, c, tag="pair 0 2")
        assert got["n_clear"][0] == 0
        # with only column 0 attached, and to arm 1: nothing of the stale track is left on arm 0's obstacle side
        cpl["src"][0][2] = -1
        _couple(pl, cpl)
        pl.tick(obs0, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
        pl.stop()
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        sh = Shared(pl, scs, cpl, live, hip_lib.pmaf_eval_order())
        kept = ref.obstacle_side(sh.paths, sh.n, sh.live, sh.tracks, None, cpl, 0, 1, sh.dt, sh.rad, 0.0, pl.cap, 1, sh.order,
                                 mutant="columns_kept")
        assert all(fv < w for fv, w in zip(kept[1][0], kept[2][0])), "the stale track was meant to cut every path of arm 0"
        got = sh.check(0, 1, c, tag="stale")
        assert got["n_clear"][0] > 0
        alone = pl.select_clear_tracked(live, 0.0, pl.cap, skip_trailing=True)
        assert alone["n_clear"][0] == 0      # (the single-population call keeps the column)
    finally:
        pl.close()


def test_every_previous_pair_in_turn(pmaf, scenes, hip_lib):
    shape, kind = "P2-N5-M3-cap9", "three"
    pl, scs, cpl = _coupled_state(pmaf, scenes, shape, kind)
    try:
        sh = Shared(pl, scs, cpl, cases.live_list(scenes, scs), hip_lib.pmaf_eval_order())
        aud, mat = sh.sides(0, 1, -0.5, 9, 1, cases.SEP, None)
        pm_mid = _median([v for row in mat[0] for v in row])
        for om, pm in ((-0.5, -0.5), (-0.5, pm_mid), (3.0, -0.5)):
            for skip in (0, 1):
                none = sh.check(0, 1, _call(9, om, pm, skip))
                for prev in ((-1, -1), (-1, 2), (3, -1)):
                    assert sh.check(0, 1, _call(9, om, pm, skip, prev=prev)) == none or np.isnan(none["cost"])
                for i in range(5):
                    for j in range(5):
                        sh.check(0, 1, _call(9, om, pm, skip, prev=(i, j)))
    finally:
        pl.close()


def test_nan_paths_never_become_the_pick(pmaf, scenes, hip_lib):
    """test_pair_clear_gpu's Had scene in both populations, each list's one field obstacle riding on the other arm:
    agents 0 and 2 have NaN paths and costs, agent 1 is finite. A NaN never wins a term, a NaN clearance is never
    feasible and takes no part in rule 2."""
    def make(p):
        sc = scenes.synthetic_scene(3, 60, 1, 9, 2)
        sc["start"] = np.array([-0.44, 0.3 * p, 0.7])
        sc["goal"] = np.array([0.6, 0.3 * p, 0.7])
        sc["obstacles"][0] = [0.0, 0.3 * p, 0.7, 0, 0, 0, 0.05]
        sc["agent_types"] = np.array([6, 1, 6], dtype=np.int32)
        return sc
    scs = [make(p) for p in range(2)]
    pl = _planner(pmaf, scs)
    try:
        pl.rollout()
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        paths, n = pl.paths()
        paths, n = np.asarray(paths).reshape(2, 3, pl.cap, 3), np.asarray(n).reshape(2, 3)
        nan_agent = [[bool(np.isnan(paths[p, a, :n[p, a]]).any()) for a in range(3)] for p in range(2)]
        assert nan_agent == [[True, False, True]] * 2
        cpl = dict(src=np.array([[1], [0]], dtype=np.int32), scale=np.array([[1.0], [0.5]]),
                   anchor=np.array([[[0.0, -0.05, 0.0]], [[0.1, 0.2, 0.35]]]), shift=0)
        _couple(pl, cpl)
        live = np.stack([s["obstacles"] for s in scs])
        sh = Shared(pl, scs, cpl, live, hip_lib.pmaf_eval_order())
        got, want = sh.whole(0, 1)
        _matrices(got, want, "NaN paths")
        assert got[2][1][1] >= 0
        for om, pm in ((-0.5, -0.5), (-0.5, -0.2)):
            for horizon in (5, 30, 61):
                for prev in (None, (0, 0), (1, 1), (2, 1)):
                    got = sh.check(0, 1, _call(horizon, om, pm, 1, prev))
                    assert got["pair"] == (1, 1) and got["rule"] in (0, 1), (om, pm, horizon, prev)
        got = sh.check(0, 1, _call(61, -0.5, 10.0, 1))          # nothing feasible: rule 2 among the non-NaN clearances only
        assert got["rule"] == 2 and not np.isnan(got["clearance"])
    finally:
        pl.close()


# ---- closed loop ----
def _dual_arm(pmaf, scenes):
    arms = scenes.dual_arm_scenes(n_agents=8, horizon=40, n_field=4)
    for s in arms:   # different gains per agent: move_real's agent_id matters too
        s["k_attr"] = np.linspace(2.0, 6.0, 8)
        s["k_damp"] = np.linspace(2.5, 4.0, 8)
    return arms, np.stack([s["start"] for s in arms])


FIELD = dict(shift=1, attach=[(0, 1.0, (-0.25, 0.0, 0.0)), (3, 0.8, (0.1, 0.0, 0.14))])


def _field_coupling(field, M):
    src = np.full((2, M), -1, dtype=np.int32)
    scale = np.ones((2, M))
    anchor = np.zeros((2, M, 3))
    for c, s, a in field["attach"]:
        src[0, c], src[1, c] = 1, 0
        scale[:, c] = s
        anchor[:, c] = a
    return dict(src=src, scale=scale, anchor=anchor, shift=field["shift"])


def test_calls_without_adoption_between_coupled_ticks_change_nothing(pmaf, scenes, hip_lib):
    """six closed-loop coupled ticks, with and without the two calls (adopt = 0, another list, offsets) in between:
    every set-point, path and rotation vector has the same bits"""
    arms, starts = _dual_arm(pmaf, scenes)
    sc = arms[0]
    cpl = _field_coupling(FIELD, 4)
    lists = [np.stack([s["obstacles"] for s in arms])]
    for t in range(6):
        nxt = np.stack([scenes.advance_live_obstacles(o) for o in lists[-1]])
        nxt[:, :-1, 3:6] = 0.02 * (t + 1)
        lists.append(nxt)
    runs = []
    for select in (False, True):
        pl = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        try:
            pl.set_initial_position(starts)
            _couple(pl, cpl)
            rec = []
            for t in range(6):
                b = pl.tick(lists[t], sc["dt"], sc["cost_gains"], sc["ws_limits"])
                rec.append((np.asarray(b).copy(), pl.last_next_pos.copy(), pl.last_next_vel.copy()))
                if select:   # given the list of the FOLLOWING tick: it must not become the resident one
                    r = pl.select_pair_clear_tracked(0, 1, lists[t + 1], 0.02, 30 if t % 2 else 1000, 0.15, 0.02,
                                                     skip_trailing=t % 3 == 0, first=None if t % 2 else [t, 1],
                                                     prev_pair=None if t == 0 else tuple(int(v) for v in b))
                    assert 0 <= r["pair"][0] < pl.N
                    clr, sp = pl.cross_audit_attached(1, 0, lists[t + 1], 0.15, sphere=True)
                    assert clr.shape == (pl.N, pl.N) and sp.min() >= 0
            pl.stop()
            rec.append((np.zeros(2), np.asarray(pl.paths()[0]).copy(), np.asarray(pl.real_known()[1]).copy()))
            runs.append(rec)
        finally:
            pl.close()
    for (b0, p0, v0), (b1, p1, v1) in zip(*runs):
        np.testing.assert_array_equal(b0, b1)
        _same_bits(p1, p0, "set-point position / paths")
        _same_bits(v1, v0, "set-point velocity / real rotation vectors")


def test_adoption_equals_adopt_best(pmaf, scenes, hip_lib):
    """two coupled handles, 6 ticks of the intended sequence: A adopts inside the call, B calls with adopt = 0 and then
    pmaf_adopt_best(pair). Results, state and set-points are bit-identical."""
    arms, starts = _dual_arm(pmaf, scenes)
    sc = arms[0]
    cpl = _field_coupling(FIELD, 4)
    obs = np.stack([s["obstacles"] for s in arms])
    A = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
    B = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
    try:
        for pl in (A, B):
            pl.set_initial_position(starts)
            _couple(pl, cpl)
            pl.start()
        prev = None
        for t in range(6):
            live = np.stack([scenes.advance_live_obstacles(o) for o in obs])
            om = (0.02, 0.06, 0.1)[t % 3]
            out = []
            for pl in (A, B):
                pl.stop()
                pl.evaluate(sc["cost_gains"], sc["ws_limits"])
                r = pl.select_pair_clear_tracked(0, 1, live, om, 30, 0.15, 0.02, skip_trailing=True, prev_pair=prev,
                                                 adopt=pl is A)
                if pl is B:
                    pl.adopt_best(np.asarray(r["pair"], dtype=np.int32))
                np.testing.assert_array_equal(pl.best()[1], np.asarray(r["pair"]) + 1)
                pl.move_real(live, sc["dt"], 1, np.asarray(r["pair"], dtype=np.int32))
                pos, vel, _ = pl.real_state()
                pl.reset_agents(pos, vel, live)
                pl.start()
                out.append(r)
            print("tick", t, out[0])
            _compare(out[0], out[1], "tick %d" % t)
            _same_state(_state(A), _state(B), "tick %d" % t)
            prev = out[0]["pair"]
            obs = live
    finally:
        A.close()
        B.close()


def test_pair_tick_clear_tracked_equals_the_explicit_sequence(pmaf, scenes, hip_lib):
    """shard.DualArmCoupling.pair_tick(field=..., clear=dict(..., tracked=True)) over 4 ticks against the calls it stands
    for; without the key it is the untracked joint call it was"""
    arms, starts = _dual_arm(pmaf, scenes)
    sc = arms[0]
    obs0 = np.stack([s["obstacles"] for s in arms])
    cpl = _field_coupling(FIELD, 4)
    for tracked in (True, False):
        A = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        B = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        try:
            ca = pmaf.shard.DualArmCoupling(obs0, 0.1)
            cb = pmaf.shard.DualArmCoupling(obs0, 0.1)
            for pl in (A, B):
                pl.set_initial_position(starts)
                pl.start()
            _couple(B, cpl)
            prev = None
            for t in range(4):
                clear = dict(margin=0.03, horizon=30, tracked=True) if tracked else dict(margin=0.03, horizon=30)
                out = ca.pair_tick(A, sc["dt"], sc["cost_gains"], sc["ws_limits"], margin=0.02, agent_radius=sc["radius"],
                                   clear=clear, adopt=True, field=FIELD)
                B.stop()
                best = B.evaluate(sc["cost_gains"], sc["ws_limits"])
                obs = cb.coupled_obstacles(B.real_state()[0])
                if tracked:
                    r = B.select_pair_clear_tracked(0, 1, obs, 0.03, 30, sc["radius"] + 0.1, 0.02, skip_trailing=True,
                                                    prev_pair=prev, adopt=True)
                else:
                    r = B.select_pair_clear(0, 1, obs, 0.03, 30, sc["radius"] + 0.1, 0.02, skip_trailing=True, prev_pair=prev,
                                            adopt=True)
                prev = r["pair"]
                assert out["rule"] == r["rule"] and out["n_feasible"] == r["n_feasible"]
                _same_bits([out["worst_excess"]], [r["worst_excess"]], "worst excess")
                pair = r["pair"] if r["pair"][0] >= 0 else tuple(int(b) for b in best)
                B.move_real(obs, sc["dt"], 1, np.asarray(pair, dtype=np.int32))
                pos, vel, _ = B.real_state()
                B.reset_agents(pos, vel, obs)
                B.start()
                print("tracked" if tracked else "untracked", "tick", t, out["pair"], pair)
                assert out["pair"] == tuple(pair)
                _same_bits([out["cost"], out["clearance"]], [r["cost"], r["clearance"]], "pair cost and clearance")
                _same_bits(out["positions"], pos, "set-points")
                _same_state(_state(A), _state(B), "tick %d" % t)
        finally:
            A.close()
            B.close()


# ---- argument errors, the abandoned-tick refusal ----
def test_argument_validation(pmaf, scenes, hip_lib):
    shape = "P2-N5-M3-cap9"
    pl, scs, cpl = _coupled_state(pmaf, scenes, shape, "one", ticks=1)
    try:
        L, h = hip_lib, pl._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        obs = np.ascontiguousarray(cases.live_list(scenes, scs), dtype=np.float64)
        oi = {k: np.full(2, -7, dtype=np.int32) for k in ("pair", "rule", "n_feasible", "n_clear", "fv", "steps")}
        od = {k: np.full(2, -7.0) for k in ("cost", "clearance", "oc", "we")}
        clr = np.full((5, 5), -7.0)
        st, sp = np.full((5, 5), -7, dtype=np.int32), np.full((5, 5), -7, dtype=np.int32)

        def outs(drop=()):
            order = ["pair", "rule", "n_feasible", "n_clear", "cost", "clearance", "oc", "fv", "we", "steps"]
            return [None if k in drop else (oi[k].ctypes.data_as(ip) if k in oi else od[k].ctypes.data_as(dp)) for k in order]

        def pair_call(h_=h, a=0, b=1, o=obs, first=None, om=0.05, horizon=5, sep=0.15, pm=0.02, prev=None, drop=()):
            fp = None if first is None else np.asarray(first, dtype=np.int32).ctypes.data_as(ip)
            pv = None if prev is None else np.asarray(prev, dtype=np.int32).ctypes.data_as(ip)
            return L.pmaf_select_pair_clear_tracked(h_, a, b, None if o is None else o.ctypes.data_as(dp), fp, om, horizon, 0, sep,
                                                    pm, pv, 0, *outs(drop))

        def audit_call(h_=h, a=0, b=1, o=obs, sep=0.15, c=clr, want_step=True, want_sphere=True):
            return L.pmaf_cross_audit_attached(h_, a, b, None if o is None else o.ctypes.data_as(dp), sep,
                                               None if c is None else c.ctypes.data_as(dp),
                                               st.ctypes.data_as(ip) if want_step else None,
                                               sp.ctypes.data_as(ip) if want_sphere else None)

        assert pair_call(h_=None) == ERR_INVALID and pair_call(o=None) == ERR_INVALID and pair_call(drop=("pair",)) == ERR_INVALID
        assert audit_call(h_=None) == ERR_INVALID and audit_call(o=None) == ERR_INVALID and audit_call(c=None) == ERR_INVALID
        for a, b in ((0, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (0, -1)):
            assert pair_call(a=a, b=b) == ERR_INVALID and audit_call(a=a, b=b) == ERR_INVALID, (a, b)
        for horizon in (0, -1, -2 ** 31):
            assert pair_call(horizon=horizon) == ERR_INVALID, horizon
        for prev in ((5, 0), (0, 5), (-2, 0), (0, -2)):
            assert pair_call(prev=prev) == ERR_INVALID, prev
        for first in ((-1, 0), (0, -1)):
            assert pair_call(first=first) == ERR_INVALID, first
        for kw in (dict(om=float("nan")), dict(pm=float("inf")), dict(sep=float("nan"))):
            assert pair_call(**kw) == ERR_INVALID, kw
        assert audit_call(sep=float("nan")) == ERR_INVALID
        bad = obs.copy()
        bad[1, 1, 6] = np.nan
        assert pair_call(o=bad) == ERR_INVALID and b"range" in L.pmaf_last_error()
        assert audit_call(o=bad) == ERR_INVALID and b"range" in L.pmaf_last_error()
        assert all((v == -7).all() for v in oi.values()) and all((v == -7.0).all() for v in od.values())   # nothing written
        assert (clr == -7.0).all() and (st == -7).all() and (sp == -7).all()
        # every optional output NULL in turn: the others unchanged
        assert pair_call(prev=(4, 4), first=(1, 0)) == 0
        full = {k: v.copy() for k, v in list(oi.items()) + list(od.items())}
        for drop in ("rule", "n_feasible", "n_clear", "cost", "clearance", "oc", "fv", "we", "steps"):
            for v in oi.values():
                v[:] = -7
            for v in od.values():
                v[:] = -7.0
            assert pair_call(prev=(4, 4), first=(1, 0), drop=(drop,)) == 0
            for k, v in list(oi.items()) + list(od.items()):
                if k == drop:
                    assert (v == -7).all(), k
                else:
                    _same_bits(v.astype(np.float64), full[k].astype(np.float64), "optional output %s without %s" % (k, drop))
        assert audit_call() == 0
        whole = (clr.copy(), st.copy(), sp.copy())
        for ws, wp in ((False, True), (True, False), (False, False)):
            clr[:], st[:], sp[:] = -7.0, -7, -7
            assert audit_call(want_step=ws, want_sphere=wp) == 0
            _same_bits(clr, whole[0], "clearance without an optional matrix")
            assert (st == (whole[1] if ws else -7)).all() and (sp == (whole[2] if wp else -7)).all()
        # offsets on a handle without tracks: PMAF_ERR_STATE, as pmaf_select_clear_tracked
        pl.couple_obstacle_tracks(None)
        assert pair_call(first=(0, 0)) == ERR_STATE and pair_call() == 0
    finally:
        pl.close()


def test_refused_after_an_abandoned_tick(pmaf, scenes, hip_lib, monkeypatch):
    """test_pair_clear_gpu's fault injection: a tick that ran into its time limit leaves the handle abandoned until
    pmaf_stop, and the joint call refuses it"""
    monkeypatch.setenv("PMAF_TICK_TIMEOUT_S", "0.002")
    scs = [scenes.synthetic_scene(512, 6000, 128, 3, 1 + p) for p in range(2)]      # ~15 ms of rollout per tick
    starts = np.stack([s["start"] for s in scs])
    obs = np.stack([s["obstacles"] for s in scs])
    sc = scs[0]
    pl = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    try:
        pl.set_initial_position(starts)
        pl.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
        pl.stop()
        pl.debug_withhold_mailbox(True)
        with pytest.raises(pmaf.PmafError) as e:
            pl.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
        assert e.value.code == -2 and "time limit" in str(e.value), str(e.value)
        pl.debug_withhold_mailbox(False)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_pair_clear_tracked(0, 1, obs, 0.05, 5, 0.15, 0.02)
        assert e.value.code == ERR_STATE, str(e.value)
        pl.stop()
        r = pl.select_pair_clear_tracked(0, 1, obs, 0.05, 5, 0.15, 0.02, adopt=True)
        assert 0 <= r["pair"][0] < 512 and 0 <= r["pair"][1] < 512
        np.testing.assert_array_equal(pl.best()[1], np.asarray(r["pair"]) + 1)
    finally:
        pl.close()
