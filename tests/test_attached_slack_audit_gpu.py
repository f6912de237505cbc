"""The joint selection on coupled handles with timing slack on the GPU (pmaf_cross_audit_attached_slack /
pmaf_select_pair_clear_tracked_slack; k_xaudit_attached_slack of csrc/pmaf_k_xattach_slack.hip) through the C-ABI, at
tolerance 0 against tests/attached_slack_reference.py on the handle's own paths, costs and composed tracks.
tests/test_attached_slack_audit.py validates the reference on the CPU, shows which rule each case is sensitive to and
asserts the pre-conditions of the behavioural case below on the same scenes. The references take the evaluation order
from pmaf_eval_order(), so the file passes unchanged under PMAF_VARIANT=rassoc.

Shapes follow the kernel's own constants (csrc/pmaf_cross_audit.hpp): T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK -- N = 5
and T + 1, capacities 9 (below one chunk) and 70 (four chunks and a ragged fifth), M = 3 and 60, P = 2 and 3; the slacks
(attached_slack_cases.slacks) sit on both sides of the chunk: (C - 1, C) leaves the diagonal chunk pair just outside the
band, (C + 1, 0) and (0, 2 C + 3) reach one and two chunks to one side only. The plain-Python reference is the slow side:
the full slack list runs on the N = 5, M = 3 shapes, N = T + 1 at two slacks, all 60 columns at one."""
import copy
import ctypes as C

import numpy as np
import pytest

import attached_audit_reference as aar
import attached_slack_cases as cases
import attached_slack_reference as ref
from test_attached_audit_gpu import (ERR_INVALID, ERR_STATE, FIELD, Shared, _call, _compare, _couple, _coupled_state, _dual_arm,
                                     _field_coupling, _median, _planner)
from test_attached_audit import tie_separation
from test_attached_slack_audit import BEHAVIOUR
from test_cross_audit_gpu import CH, T
from test_select_clear_gpu import _same_bits, _same_state, _state

pytestmark = pytest.mark.gpu


def test_the_shapes_and_slacks_follow_the_kernel_constants():
    assert cases.T == T and cases.C == CH and cases.SHAPES["P2-N33-M3-cap70-ragged"]["N"] == T + 1
    assert 9 < CH and 70 > 4 * CH and 70 % CH != 0
    assert cases.LATE_CAP > CH and cases.LATE_CAP % CH != 0


def _matrices(got, want, tag):
    _same_bits(got[0], want[0], tag + " clearance")
    for k, name in ((1, "step_a"), (2, "step_b"), (3, "sphere")):
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg=tag + " " + name)


class SlackShared(Shared):
    """test_attached_audit_gpu.Shared with a slack: the reference's matrices of one handle state, computed once per key
    and never modified"""

    def __init__(self, *a):
        super().__init__(*a)
        self.smat = {}

    def want(self, a, b, c, sep, first=None, late=None):
        if late is None:
            return super().want(a, b, c, sep, first)
        aud, _ = self.sides(a, b, c["obstacle_margin"], c["horizon"], c["skip_trailing"], sep, first)
        km = (a, b, c["horizon"], sep, tuple(late))
        if km not in self.smat:
            self.smat[km] = ref.pair_side(self.paths[a], self.n[a], self.paths[b], self.n[b], self.cpl, a, b, self.live,
                                          self.rad, c["horizon"], sep, late, self.order)
        return ref.select_pair_clear_tracked_slack(self.paths, self.n, self.live, self.tracks, first, self.cpl, self.costs,
                                                   self.dt, self.rad, a, b, c["obstacle_margin"], c["horizon"],
                                                   c["skip_trailing"], sep, c["pair_margin"], late, c["prev_pair"], self.order,
                                                   aud, self.smat[km])

    def call(self, a, b, c, sep, first=None, adopt=False, late=None):
        return self.pl.select_pair_clear_tracked(a, b, self.live, c["obstacle_margin"], c["horizon"], sep, c["pair_margin"],
                                                 skip_trailing=c["skip_trailing"], prev_pair=c["prev_pair"], adopt=adopt,
                                                 first=first, late=late)

    def check(self, a, b, c, sep=cases.SEP, first=None, tag="", late=None):
        got = self.call(a, b, c, sep, first, late=late)
        _compare(got, self.want(a, b, c, sep, first, late), "%s %r first %r late %r" % (tag, c, first, late))
        return got

    def whole(self, a, b, late, sep=cases.SEP):
        """the slacked attached audit on the whole paths, device and reference"""
        got = self.pl.cross_audit_attached_slack(a, b, self.live, sep, late[0], late[1], steps=True, sphere=True)
        want = ref.cross_audit_attached_slack(self.paths[a], self.n[a], self.paths[b], self.n[b], self.cpl, a, b, self.live,
                                              self.rad, sep, late[0], late[1], self.order)
        return got, want


def _device(pl, live, late, a=0, b=1, sep=cases.SEP):
    return pl.cross_audit_attached_slack(a, b, live, sep, late[0], late[1], steps=True, sphere=True)


# ---- the matrices: every shape, attachment kind and slack the kernel can go wrong at ----
SMALL = [s for s in cases.SHAPES if cases.SHAPES[s]["N"] == 5 and cases.SHAPES[s]["M"] == 3]
MATRIX_CASES = [(s, k, "full") for s in SMALL for k in ("none", "one", "tie", "three")]
MATRIX_CASES += [("P2-N33-M3-cap70-ragged", "one", "two"), ("P2-N5-M60-cap70-general-ragged", "three", "one"),
                 ("P2-N5-M60-cap70-general-ragged", "all", "one")]


@pytest.mark.parametrize("shape,kind,slacks", MATRIX_CASES, ids=lambda v: str(v))
def test_matrices_at_every_slack(pmaf, scenes, hip_lib, shape, kind, slacks):
    s = cases.SHAPES[shape]
    pl, scs, cpl = _coupled_state(pmaf, scenes, shape, kind)
    try:
        cap, M = s["cap"], s["M"]
        live = cases.live_list(scenes, scs)
        sh = SlackShared(pl, scs, cpl, live, hip_lib.pmaf_eval_order())
        if s["ragged"]:
            assert len(set(sh.n[1])) > 1, "the ragged case is meant to have paths of different lengths"
        lates = {"full": cases.slacks(cap), "two": [(3, 2), (CH + 1, 0)], "one": [(3, 2)]}[slacks]
        by_late = {}
        for late in lates:
            if late[0] >= 10 ** 6:      # the clamp: far beyond everything equals everything, device against device
                got = _device(pl, live, late)
                _matrices(got, by_late[(cap, cap)], "%s %s clamp" % (shape, kind))
                continue
            got, want = sh.whole(0, 1, late)
            _matrices(got, want, "%s %s late %r" % (shape, kind, late))
            by_late[late] = got
            sp, sa, sb = np.asarray(got[3]), np.asarray(got[1]), np.asarray(got[2])
            print(shape, kind, late, "sphere codes that win:", sorted(set(sp.reshape(-1).tolist())),
                  "pairs won by a sphere at two different steps:", int(((sp > 0) & (sa != sb)).sum()))
            assert ((sb - sa <= late[0]) & (sa - sb <= late[1])).all()
        if (0, 0) in by_late:      # device against device: the attached audit, through another kernel
            clr, st, sp = pl.cross_audit_attached(0, 1, live, cases.SEP, step=True, sphere=True)
            got = by_late[(0, 0)]
            _same_bits(got[0], clr, "pmaf_cross_audit_attached")
            np.testing.assert_array_equal(got[1], st)
            np.testing.assert_array_equal(got[2], st)
            np.testing.assert_array_equal(got[3], sp)
        if kind == "tie":          # a tie in d2, (k, l) AND the gap between term 0 and term 1: the smallest term keeps it
            sep = tie_separation(scs, sh.live)
            got, want = sh.whole(0, 1, (3, 2), sep)
            _matrices(got, want, "%s tie separation" % shape)
            assert 1 not in np.asarray(got[3]) and (np.asarray(got[3]) == 0).any()
        if kind == "none":         # device against device: the slacked audit
            for late in lates:
                clr, sa, sb = pl.cross_audit_slack(0, 1, cases.SEP, late[0], late[1], steps=True)
                got = _device(pl, live, late)
                _same_bits(got[0], clr, "pmaf_cross_audit_slack %r" % (late,))
                np.testing.assert_array_equal(got[1], sa)
                np.testing.assert_array_equal(got[2], sb)
                assert (np.asarray(got[3]) == np.where(sa >= 0, 0, -1)).all()
        # the clearance never grows with a slack
        chain = [l for l in cases.chain(cap) if l in by_late]
        for lo, hi in zip(chain, chain[1:]):
            assert (np.asarray(by_late[hi][0]) <= np.asarray(by_late[lo][0])).all(), (lo, hi)
        # the transposed call: the same clearance bits, the codes swapped (no two terms tie in the gap but in `tie`)
        for late in [l for l in ((3, 2), (0, 2 * CH + 3)) if l in by_late]:
            t = _device(pl, live, (late[1], late[0]), 1, 0)
            _same_bits(np.asarray(t[0]).T, by_late[late][0], "transposed %r" % (late,))
            if kind != "tie":
                c = np.asarray(by_late[late][3])
                np.testing.assert_array_equal(np.asarray(t[3]).T, np.where(c <= 0, c, np.where(c <= M, c + M, c - M)))
    finally:
        pl.close()


def test_each_output_pointer_null_in_turn(pmaf, scenes, hip_lib):
    shape = "P2-N5-M3-cap70-ragged"
    pl, scs, cpl = _coupled_state(pmaf, scenes, shape, "three", ticks=1)
    try:
        L, h = hip_lib, pl._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        obs = np.ascontiguousarray(cases.live_list(scenes, scs), dtype=np.float64)
        clr = np.full((5, 5), -7.0)
        ints = [np.full((5, 5), -7, dtype=np.int32) for _ in range(3)]

        def audit(keep=(True, True, True), c=clr, a=0, b=1, la=3, lb=2, h_=h, o=obs, sep=0.15):
            return L.pmaf_cross_audit_attached_slack(h_, a, b, None if o is None else o.ctypes.data_as(dp), sep, la, lb,
                                                     None if c is None else c.ctypes.data_as(dp),
                                                     *[m.ctypes.data_as(ip) if k else None for m, k in zip(ints, keep)])

        assert audit(h_=None) == ERR_INVALID and audit(o=None) == ERR_INVALID and audit(c=None) == ERR_INVALID
        for a, b in ((0, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (0, -1)):
            assert audit(a=a, b=b) == ERR_INVALID, (a, b)
        for la, lb in ((-1, 0), (0, -1), (-2 ** 31, 3)):
            assert audit(la=la, lb=lb) == ERR_INVALID and b"late" in L.pmaf_last_error(), (la, lb)
        assert audit(sep=float("nan")) == ERR_INVALID
        bad = obs.copy()
        bad[1, 1, 6] = np.nan
        assert audit(o=bad) == ERR_INVALID and b"range" in L.pmaf_last_error()
        assert (clr == -7.0).all() and all((m == -7).all() for m in ints)      # nothing written
        assert audit() == 0
        full = (clr.copy(), [m.copy() for m in ints])
        assert (full[1][0] != full[1][1]).any() and (full[1][2] > 0).any()
        for keep in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, True, True),
                     (False, False, False), (True, False, False)):
            clr[:] = -7.0
            for m in ints:
                m[:] = -7
            assert audit(keep) == 0
            _same_bits(clr, full[0], "clearance with %r" % (keep,))
            for m, f, k in zip(ints, full[1], keep):
                assert (m == (f if k else -7)).all(), keep
    finally:
        pl.close()


# ---- the joint call: every rule and n_feasible regime, late NULL and given ----
JOINT_CASES = [(s, k) for s in SMALL for k in ("none", "one", "three")]
_SEEN = {}


def _run_joint(pmaf, scenes, hip_lib, shape, kind):
    if (shape, kind) in _SEEN:
        return _SEEN[(shape, kind)]
    s = cases.SHAPES[shape]
    pl, scs, cpl = _coupled_state(pmaf, scenes, shape, kind)
    seen = set()
    try:
        N, cap = s["N"], s["cap"]
        live = cases.live_list(scenes, scs)
        sh = SlackShared(pl, scs, cpl, live, hip_lib.pmaf_eval_order())
        k = 0
        for horizon in (3, cap // 2, cap + 6):
            for skip in (0, 1):
                aud, _ = sh.sides(0, 1, -0.5, horizon, skip, cases.SEP, None)
                late = (3, 2) if horizon != 3 else (1, 0)
                wide = sh.want(0, 1, _call(horizon, -0.5, -0.5, skip), cases.SEP, None, late)      # (fills sh.smat)
                mat = sh.smat[(0, 1, horizon, cases.SEP, late)]
                om_mid = _median(aud[0][0] + aud[0][1])
                pm_mid = _median([v for row in mat[0] for v in row])
                for om, pm in ((-0.5, -0.5), (3.0, -0.5), (-0.5, 3.0), (om_mid, pm_mid), (-0.5, pm_mid)):
                    prev = ((3 * k) % N, (5 * k + 1) % N) if k % 2 else None
                    first = [k % 3, (k + 1) % 4] + [0] * (pl.P - 2) if (sh.tracked and k % 3 == 1) else None
                    c = _call(horizon, om, pm, skip, prev)
                    r = sh.check(0, 1, c, first=first, tag="%s %s" % (shape, kind), late=late)
                    seen.add((r["rule"], 0 if r["n_feasible"] == 0 else (2 if r["n_feasible"] == N * N else 1)))
                    if r["pair"][0] >= 0:
                        assert -late[1] <= r["steps"][1] - r["steps"][0] <= late[0]
                    # late NULL: pmaf_select_pair_clear_tracked exactly, device against device and against its reference
                    u = pl.select_pair_clear_tracked(0, 1, live, om, horizon, cases.SEP, pm, skip_trailing=skip, prev_pair=prev,
                                                     first=first)
                    null = L_null(pl, hip_lib, live, c, first)
                    _compare(null, u, "late NULL %r" % (c,))
                    if kind == "none":      # nothing rides: the untracked joint call with the same slack
                        if first is None:
                            v = pl.select_pair_clear(0, 1, live, om, horizon, cases.SEP, pm, skip_trailing=skip, late=late,
                                                     prev_pair=prev)
                            _compare(r, v, "pmaf_select_pair_clear(late) %r" % (c,))
                    k += 1
                assert wide["pair"][0] >= 0 or np.isnan(wide["cost"])
        if pl.P > 2:      # the third population's column stays on the obstacle side; population offsets with a > b
            for a, b in ((1, 0), (2, 0), (1, 2)):
                got, want = sh.whole(a, b, (3, 2))
                _matrices(got, want, "%s %s pops %d %d" % (shape, kind, a, b))
                r = sh.check(a, b, _call(cap, 0.0, 0.0, 1, (1, 2)), tag="pops %d %d" % (a, b), late=(3, 2))
                u = sh.check(a, b, _call(cap, 0.0, 0.0, 1, (1, 2)), tag="pops %d %d" % (a, b))
                assert r["n_clear"] == u["n_clear"]      # the obstacle side does not see the slack
    finally:
        pl.close()
    _SEEN[(shape, kind)] = seen
    return seen


def L_null(pl, L, live, c, first):
    """pmaf_select_pair_clear_tracked_slack with late == NULL, through the C-ABI (the binding's late=None calls the
    un-slacked export)"""
    o, args = pl._joint_outputs()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    obs = np.ascontiguousarray(live, dtype=np.float64)
    fp = None if first is None else np.ascontiguousarray(first, dtype=np.int32)
    pv = None if c["prev_pair"] is None else np.ascontiguousarray(c["prev_pair"], dtype=np.int32)
    rc = L.pmaf_select_pair_clear_tracked_slack(pl._h, 0, 1, obs.ctypes.data_as(dp), None if fp is None else fp.ctypes.data_as(ip),
                                                float(c["obstacle_margin"]), int(c["horizon"]), int(c["skip_trailing"]),
                                                float(cases.SEP), float(c["pair_margin"]), None,
                                                None if pv is None else pv.ctypes.data_as(ip), 0, *args)
    assert rc == 0, L.pmaf_last_error()
    return pl._joint_dict(o)


@pytest.mark.parametrize("shape,kind", JOINT_CASES, ids=lambda v: str(v))
def test_joint_call_horizons_margins_slacks(pmaf, scenes, hip_lib, shape, kind):
    seen = _run_joint(pmaf, scenes, hip_lib, shape, kind)
    print("(rule, n_feasible regime) seen:", sorted(seen))
    assert seen


def test_every_rule_and_every_n_feasible_regime_occurred(pmaf, scenes, hip_lib):
    seen = set()
    for shape, kind in JOINT_CASES:
        seen |= _run_joint(pmaf, scenes, hip_lib, shape, kind)
    print("(rule, n_feasible regime) over the whole parametrisation:", sorted(seen))
    assert {r for r, _ in seen} == {0, 1, 2}
    assert {g for _, g in seen} == {0, 1, 2}     # no pair feasible, some, all


# ---- the case that fails without the feature, and its mirror ----
@pytest.mark.parametrize("side", [0, 1])
def test_a_late_arm_runs_into_the_riding_sphere(pmaf, scenes, hip_lib, side):
    """dt = 0.1. After a rollout the joint calls pick (i*, j*). Column 0 of A's list (side 0; of B's: side 1) is attached
    with scale 1 and an anchor that puts the sphere riding on one member, d steps LATER, on the other member's point. Step
    against step the pair stays feasible and pmaf_select_pair_clear_tracked returns it. With the slack that lets the arm
    run late, the new call does not, and equals the reference; the same lag the wrong way round keeps the pair.
    (tests/test_attached_slack_audit.py asserts the same on the oracle's rollouts of these scenes.)"""
    scs = cases.build_scenes(scenes, cases.LATE_SHAPE)
    pl = _planner(pmaf, scs)
    try:
        pl.rollout()
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        live = cases.live_list(scenes, scs)
        b, cap, d = BEHAVIOUR, pl.cap, cases.LATE_D
        assert cap == cases.LATE_CAP
        plain = pl.select_pair_clear(0, 1, live, b["obstacle_margin"], cap, cases.SEP, b["pair_margin"],
                                     skip_trailing=b["skip_trailing"])
        assert plain["rule"] in (0, 1) and plain["pair"][0] >= 0, plain
        star = plain["pair"]
        paths, n = pl.paths()
        paths, n = np.asarray(paths).reshape(2, pl.N, cap, 3), np.asarray(n).reshape(2, pl.N)
        k = cases.late_step(n)
        cpl = cases.sphere_on_the_late_pair(2, pl.n_obs - 1, paths, n, star, k, d, side)
        far = cases.late_rows(live, cpl)
        _couple(pl, cpl)
        sh = SlackShared(pl, scs, cpl, far, hip_lib.pmaf_eval_order())
        c = _call(cap, b["obstacle_margin"], b["pair_margin"], b["skip_trailing"])
        tracked = sh.check(0, 1, c, tag="step against step")
        assert tracked["pair"] == star and tracked["rule"] in (0, 1)
        hit, wrong = cases.late_slack(side), cases.late_slack(side, wrong=True)
        got = sh.check(0, 1, c, tag="late", late=hit)
        print("un-slacked", tracked["pair"], tracked["n_feasible"], "slacked", got["pair"], got["rule"], got["n_feasible"])
        assert got["pair"] != star
        assert sh.check(0, 1, c, tag="the wrong way round", late=wrong)["pair"] == star
        i, j = star
        code = 1 if side == 0 else 1 + (pl.n_obs - 1)
        clr, sa, sb, sp = _device(pl, far, hit)
        assert sp[i][j] == code and clr[i][j] < 0.0
        assert (sa[i][j], sb[i][j]) == ((k, k + d) if side == 0 else (k + d, k))
        assert _device(pl, far, (0, 0))[0][i][j] > 0.0 and _device(pl, far, wrong)[0][i][j] > 0.0
        for late in ((0, 0), hit, wrong, (cap, cap)):
            _matrices(*sh.whole(0, 1, late), "behaviour %r" % (late,))
    finally:
        pl.close()


def test_a_tie_inside_a_term_goes_to_the_least_k_then_l(pmaf, scenes, hip_lib):
    """twin scenes: both populations have the same paths, and a sphere with scale -1 makes the minimum of the pair (0, 0)
    occur at (ka, kb) and at (kb, ka) with the same bits (attached_slack_cases.twin_coupling); the kernel visits the
    chunk pairs in another order than (k, l) and must still report (ka, kb)"""
    shape = "P2-N5-M3-cap70-ragged"
    scs = cases.build_scenes(scenes, shape)
    scs[1] = copy.deepcopy(scs[0])
    pl = _planner(pmaf, scs)
    try:
        pl.rollout()
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        paths, n = pl.paths()
        paths, n = np.asarray(paths).reshape(2, pl.N, pl.cap, 3), np.asarray(n).reshape(2, pl.N)
        assert (paths[0] == paths[1]).all() and (n[0] == n[1]).all()
        live = cases.live_list(scenes, scs)
        for gap in (2, CH + 1):      # inside one chunk pair, and across two chunks of B
            cpl, ka, kb = cases.twin_coupling(2, pl.n_obs - 1, paths, n, 0, gap)
            _couple(pl, cpl)
            sh = SlackShared(pl, scs, cpl, live, hip_lib.pmaf_eval_order())
            for late in ((gap, gap), (pl.cap, pl.cap)):
                got, want = sh.whole(0, 1, late, cases.TWIN_SEP)
                _matrices(got, want, "twin %d %r" % (gap, late))
                print("twin", gap, late, [np.asarray(m)[0][0] for m in got])
                assert (got[1][0][0], got[2][0][0], got[3][0][0]) == (ka, kb, 1)
    finally:
        pl.close()


def test_nan_paths_never_win(pmaf, scenes, hip_lib):
    """test_attached_audit_gpu's NaN scene: agents 0 and 2 have NaN paths and costs, agent 1 is finite"""
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
        assert [[bool(np.isnan(paths[p, a, :n[p, a]]).any()) for a in range(3)] for p in range(2)] == [[True, False, True]] * 2
        cpl = dict(src=np.array([[1], [0]], dtype=np.int32), scale=np.array([[1.0], [0.5]]),
                   anchor=np.array([[[0.0, -0.05, 0.0]], [[0.1, 0.2, 0.35]]]), shift=0)
        _couple(pl, cpl)
        live = np.stack([s["obstacles"] for s in scs])
        sh = SlackShared(pl, scs, cpl, live, hip_lib.pmaf_eval_order())
        for late in ((0, 0), (3, 2), (CH + 1, 0)):
            got, want = sh.whole(0, 1, late)
            _matrices(got, want, "NaN paths %r" % (late,))
            assert got[3][1][1] >= 0
        for om, pm in ((-0.5, -0.5), (-0.5, -0.2)):
            for horizon in (5, 61):
                for prev in (None, (0, 0), (2, 1)):
                    got = sh.check(0, 1, _call(horizon, om, pm, 1, prev), late=(3, 2))
                    assert got["pair"] == (1, 1) and got["rule"] in (0, 1), (om, pm, horizon, prev)
        got = sh.check(0, 1, _call(61, -0.5, 10.0, 1), late=(3, 2))      # nothing feasible: rule 2 among the non-NaN only
        assert got["rule"] == 2 and not np.isnan(got["clearance"])
    finally:
        pl.close()


# ---- closed loop ----
def test_adoption_equals_adopt_best(pmaf, scenes, hip_lib):
    """two coupled handles, 4 ticks: A adopts inside the slacked call, B calls with adopt = 0 and then
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
        for t in range(4):
            live = np.stack([scenes.advance_live_obstacles(o) for o in obs])
            out = []
            for pl in (A, B):
                pl.stop()
                pl.evaluate(sc["cost_gains"], sc["ws_limits"])
                r = pl.select_pair_clear_tracked(0, 1, live, (0.02, 0.06)[t % 2], 30, 0.15, 0.02, skip_trailing=True,
                                                 prev_pair=prev, adopt=pl is A, late=(3, 2))
                if pl is B:
                    pl.adopt_best(np.asarray(r["pair"], dtype=np.int32))
                np.testing.assert_array_equal(pl.best()[1], np.asarray(r["pair"]) + 1)
                pl.move_real(live, sc["dt"], 1, np.asarray(r["pair"], dtype=np.int32))
                pos, vel, _ = pl.real_state()
                pl.reset_agents(pos, vel, live)
                pl.start()
                out.append(r)
            _compare(out[0], out[1], "tick %d" % t)
            _same_state(_state(A), _state(B), "tick %d" % t)
            prev = out[0]["pair"]
            obs = live
    finally:
        A.close()
        B.close()


def test_pair_tick_clear_tracked_late_equals_the_explicit_sequence(pmaf, scenes, hip_lib):
    """six closed-loop coupled ticks through shard.DualArmCoupling.pair_tick(field=..., clear=dict(..., tracked=True),
    late=(3, 2)) against the calls it stands for, each selection also against the reference"""
    arms, starts = _dual_arm(pmaf, scenes)
    sc = arms[0]
    obs0 = np.stack([s["obstacles"] for s in arms])
    cpl = _field_coupling(FIELD, 4)
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
        for t in range(6):
            out = ca.pair_tick(A, sc["dt"], sc["cost_gains"], sc["ws_limits"], margin=0.02, agent_radius=sc["radius"],
                               clear=dict(margin=0.03, horizon=30, tracked=True), adopt=True, field=FIELD, late=(3, 2))
            B.stop()
            best = B.evaluate(sc["cost_gains"], sc["ws_limits"])
            obs = cb.coupled_obstacles(B.real_state()[0])
            sh = SlackShared(B, arms, cpl, obs, hip_lib.pmaf_eval_order())
            c = _call(30, 0.03, 0.02, 1, prev)
            want = sh.want(0, 1, c, sc["radius"] + 0.1, None, (3, 2))
            r = sh.call(0, 1, c, sc["radius"] + 0.1, adopt=True, late=(3, 2))
            _compare(r, want, "tick %d" % t)
            prev = r["pair"]
            assert out["rule"] == r["rule"] and out["n_feasible"] == r["n_feasible"] and out["steps"] == r["steps"]
            pair = r["pair"] if r["pair"][0] >= 0 else tuple(int(b) for b in best)
            B.move_real(obs, sc["dt"], 1, np.asarray(pair, dtype=np.int32))
            pos, vel, _ = B.real_state()
            B.reset_agents(pos, vel, obs)
            B.start()
            print("tick", t, out["pair"], out["rule"], out["steps"], out["clearance"])
            assert out["pair"] == tuple(pair)
            _same_bits([out["cost"], out["clearance"]], [r["cost"], r["clearance"]], "pair cost and clearance")
            _same_bits(out["positions"], pos, "set-points")
            _same_state(_state(A), _state(B), "tick %d" % t)
    finally:
        A.close()
        B.close()


# ---- argument errors, the clamp, the abandoned-tick refusal ----
def test_joint_call_validation_and_the_clamp(pmaf, scenes, hip_lib):
    shape = "P2-N5-M3-cap9"
    pl, scs, cpl = _coupled_state(pmaf, scenes, shape, "one", ticks=1)
    try:
        live = cases.live_list(scenes, scs)
        for late in ((-1, 0), (0, -1)):
            with pytest.raises(pmaf.PmafError) as e:
                pl.select_pair_clear_tracked(0, 1, live, 0.05, 5, 0.15, 0.02, late=late)
            assert e.value.code == ERR_INVALID and "late" in str(e.value)
        for a, b in ((0, 0), (1, 1), (0, 2), (-1, 0)):
            with pytest.raises(pmaf.PmafError) as e:
                pl.select_pair_clear_tracked(a, b, live, 0.05, 5, 0.15, 0.02, late=(1, 1))
            assert e.value.code == ERR_INVALID
        for kw in (dict(horizon=0), dict(prev_pair=(5, 0)), dict(first=(-1, 0))):
            args = dict(obstacle_margin=0.05, horizon=5, separation=0.15, pair_margin=0.02, late=(1, 1))
            args.update(kw)
            with pytest.raises(pmaf.PmafError) as e:
                pl.select_pair_clear_tracked(0, 1, live, **args)
            assert e.value.code == ERR_INVALID, kw
        # a slack of max_prediction_steps or more admits every pair of steps
        want = pl.select_pair_clear_tracked(0, 1, live, 0.0, pl.cap, 0.15, 0.0, late=(pl.cap, pl.cap))
        for late in ((10 ** 6, 10 ** 6), (2 ** 31 - 1, pl.cap)):
            _compare(pl.select_pair_clear_tracked(0, 1, live, 0.0, pl.cap, 0.15, 0.0, late=late), want, "clamp %r" % (late,))
        # offsets on a handle without tracks: PMAF_ERR_STATE, as pmaf_select_clear_tracked
        pl.couple_obstacle_tracks(None)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_pair_clear_tracked(0, 1, live, 0.05, 5, 0.15, 0.02, first=(0, 0), late=(1, 1))
        assert e.value.code == ERR_STATE
    finally:
        pl.close()


def test_refused_after_an_abandoned_tick(pmaf, scenes, hip_lib, monkeypatch):
    """test_attached_audit_gpu's host-side time limit: a tick that ran into it leaves the handle abandoned until
    pmaf_stop, and the slacked joint call refuses it like the un-slacked one"""
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
            pl.select_pair_clear_tracked(0, 1, obs, 0.05, 5, 0.15, 0.02, late=(1, 1))
        assert e.value.code == ERR_STATE, str(e.value)
        pl.stop()
        r = pl.select_pair_clear_tracked(0, 1, obs, 0.05, 5, 0.15, 0.02, adopt=True, late=(1, 1))
        assert 0 <= r["pair"][0] < 512 and 0 <= r["pair"][1] < 512
        np.testing.assert_array_equal(pl.best()[1], np.asarray(r["pair"]) + 1)
    finally:
        pl.close()


# ---- one handle, every kind of call in turn: the scratch layout grows and is shared ----
def test_alternating_calls_of_every_kind_on_one_handle(pmaf, scenes, hip_lib):
    """the cross-audit and joint calls share one grow-only scratch whose layout depends on the call (the slacked attached
    audit's sphere matrix lies behind everything else). Every kind is called on two handles in the same state in
    different orders, the cheap layouts first on one and last on the other, results compared after every call."""
    shape = "P2-N5-M3-cap70-ragged"

    def calls(pl, live, tracks, nt):
        j = dict(skip_trailing=True, prev_pair=(1, 2))
        return [
            ("cross_audit", lambda: pl.cross_audit(0, 1, cases.SEP, step=True)),
            ("cross_audit_tracks", lambda: pl.cross_audit_tracks(0, tracks, nt, cases.SEP, step=True)),
            ("select_pair", lambda: pl.select_pair(0, 1, cases.SEP, 0.0)),
            ("cross_audit_slack", lambda: pl.cross_audit_slack(0, 1, cases.SEP, 3, 2, steps=True)),
            ("cross_audit_tracks_slack", lambda: pl.cross_audit_tracks_slack(0, tracks, nt, cases.SEP, 3, 2, steps=True)),
            ("select_pair_slack", lambda: pl.select_pair_slack(0, 1, cases.SEP, 0.0, 3, 2)),
            ("cross_audit_attached", lambda: pl.cross_audit_attached(0, 1, live, cases.SEP, step=True, sphere=True)),
            ("cross_audit_attached_slack", lambda: pl.cross_audit_attached_slack(0, 1, live, cases.SEP, 3, 2, steps=True, sphere=True)),
            ("cross_audit_attached_slack/no sphere", lambda: pl.cross_audit_attached_slack(0, 1, live, cases.SEP, 3, 2, steps=True)),
            ("select_pair_clear", lambda: pl.select_pair_clear(0, 1, live, 0.0, 40, cases.SEP, 0.0, late=(3, 2), **j)),
            ("select_clear_tracks", lambda: pl.select_clear_tracks(0, live, 0.0, 40, tracks, nt, cases.SEP, 0.0, late=(3, 2), **j)),
            ("select_pair_clear_tracked", lambda: pl.select_pair_clear_tracked(0, 1, live, 0.0, 40, cases.SEP, 0.0, **j)),
            ("select_pair_clear_tracked_slack", lambda: pl.select_pair_clear_tracked(0, 1, live, 0.0, 40, cases.SEP, 0.0, late=(3, 2), **j)),
        ]

    def flat(r):
        if isinstance(r, dict):
            return [np.asarray(r[k], dtype=np.float64) for k in sorted(r)]
        return [np.asarray(m, dtype=np.float64) for m in (r if isinstance(r, tuple) else (r,))]

    def state():
        pl, scs, cpl = _coupled_state(pmaf, scenes, shape, "three")
        live = cases.live_list(scenes, scs)
        paths, n = pl.paths()
        tracks = np.ascontiguousarray(np.asarray(paths).reshape(2, pl.N, pl.cap, 3)[1][:3])
        nt = np.ascontiguousarray(np.asarray(n).reshape(2, pl.N)[1][:3])
        return pl, calls(pl, live, tracks, nt)

    # two handles in the same state: on one the cheap layouts come first, on the other the slacked attached audit's
    X, cx = state()
    Y, cy = state()
    try:
        want = {}
        order = list(range(len(cx)))
        for k in order:
            want[cx[k][0]] = flat(cx[k][1]())
        for pl_calls, seqs in ((cy, (order[::-1], order)), (cx, ([(5 * i + 3) % len(cx) for i in order], order[::-1]))):
            for seq in seqs:
                assert sorted(seq) == order
                for k in seq:
                    for g, w in zip(flat(pl_calls[k][1]()), want[pl_calls[k][0]]):
                        _same_bits(g, w, pl_calls[k][0])
    finally:
        X.close()
        Y.close()
