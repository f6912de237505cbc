"""Cross audit with timing slack on the GPU (pmaf_cross_audit_slack / pmaf_cross_audit_tracks_slack /
pmaf_select_pair_slack, include/pmaf.h) through the C-ABI against tests/slack_audit_reference.py at TOLERANCE 0: integers
equal, doubles bit-equal, a NaN matched by a NaN; no case is skipped. The reference takes its dot association from
pmaf_eval_order(), so the file passes unchanged under PMAF_VARIANT=rassoc.

Fixtures and shapes are those of tests/test_cross_audit_gpu.py (T = the tile edge, CH = the step chunk of the kernels,
read from csrc/pmaf_cross_audit.hpp): N = T + 1 needs a second, ragged tile in both directions, a horizon of CH + 6 a
second, ragged chunk. The slacks walk the kernel's paths: (0, 0) one masked chunk pair per chunk; (1, 0) / (0, 1) / (3, 2)
a neighbouring chunk's edge; (CH - 1, CH) and (CH + 1, 0) chunk pairs wholly inside the band next to edge ones; cap and
10^6 every pair of steps and the host's clamp."""
import ctypes as C

import numpy as np
import pytest

import cross_audit_reference as ref
import slack_audit_reference as sref
from test_cross_audit_gpu import CH, SEP, T, _paths, _results, coupled_handle, rest_pair
from test_path_audit_gpu import _same_bits, rollout_case

pytestmark = pytest.mark.gpu


def slacks(cap):
    return [(0, 0), (1, 0), (0, 1), (3, 2), (CH - 1, CH), (CH + 1, 0), (cap, cap), (10 ** 6, 10 ** 6)]


def check_slacked(pl, a, b, late, hip_lib, sep=SEP):
    """pmaf_cross_audit_slack(a, b) against the reference on the handle's own paths; returns the reference's
    (clearance, step_a, step_b) as arrays"""
    paths, n = _paths(pl)
    want = sref.cross_audit_slack(paths[a].tolist(), n[a].tolist(), paths[b].tolist(), n[b].tolist(), sep, late[0], late[1],
                                  hip_lib.pmaf_eval_order())
    got_c, got_a, got_b = pl.cross_audit_slack(a, b, sep, late[0], late[1], steps=True)
    np.testing.assert_array_equal(got_a, np.asarray(want[1], dtype=np.int32), err_msg="step_a at slack %s" % (late,))
    np.testing.assert_array_equal(got_b, np.asarray(want[2], dtype=np.int32), err_msg="step_b at slack %s" % (late,))
    _same_bits(got_c, want[0], "clearance at slack %s" % (late,))
    _same_bits(pl.cross_audit_slack(a, b, sep, late[0], late[1]), want[0], "clearance without steps at slack %s" % (late,))
    return tuple(np.asarray(w) for w in want)


@pytest.mark.parametrize("P,N,H,pops,ragged", [(2, 1, 8, (0, 1), False), (2, 5, CH + 6, (1, 0), False),
                                               (2, T + 1, 8, (0, 1), False), (3, T + 1, CH + 6, (2, 0), False),
                                               (2, 5, 70, (0, 1), True), (3, 5, 8, (2, 0), False)])
def test_matrix_and_steps_against_the_reference(pmaf, scenes, hip_lib, P, N, H, pops, ragged):
    pl, scs, _ = rollout_case(pmaf, scenes, P, N, 2, H, ragged)
    try:
        a, b = pops
        _, n = _paths(pl)
        cap = pl.cap
        if ragged:
            for p in (a, b):
                assert len(set(n[p].tolist())) > 1, "the case is meant to have paths of different lengths in both sets: %s" % n
            assert n.min() < cap
        else:
            assert (n == cap).all()
        big_k = np.maximum(n[a][:, None], n[b][None, :])
        want = {}
        for late in slacks(cap):
            c, sa, sb = want[late] = check_slacked(pl, a, b, late, hip_lib)
            print("slack", late, "clearance", c.min(), c.max(), "step_a", sa.min(), sa.max(), "step_b", sb.min(), sb.max())
            assert (sa >= 0).all() and (sa < big_k).all() and (sb >= 0).all() and (sb < big_k).all()
            assert (sb - sa <= late[0]).all() and (sa - sb <= late[1]).all()
            # the mirrored call: the transposed clearance bits
            _same_bits(pl.cross_audit_slack(b, a, SEP, late[1], late[0]).T, c, "transpose of (B, A) at slack %s" % (late,))
        # (these populations start next to each other and part: the closest pair of steps is mostly (0, 0) at every slack;
        # the dual-arm case below is the one where the slack decides)
        lower = int((want[3, 2][0] < want[0, 0][0]).sum())
        print("pairs strictly closer at (3, 2) than at (0, 0):", lower, "of", want[0, 0][0].size)
        assert (want[3, 2][0] <= want[0, 0][0]).all()
        _same_bits(want[cap, cap][0], want[10 ** 6, 10 ** 6][0], "every pair of steps")
    finally:
        pl.close()


def test_dual_arm_paths_where_the_slack_decides(pmaf, scenes, hip_lib):
    """the two arms of scenes.dual_arm_scenes pass each other: by the REFERENCE's numbers some pairs are strictly closer
    at slack (3, 2) than step against step, so the suite cannot pass on inputs for which the slack never matters"""
    pl, arms, starts = coupled_handle(pmaf, scenes, 5, 60)
    try:
        pl.rollout()
        want = {late: check_slacked(pl, 0, 1, late, hip_lib) for late in slacks(pl.cap)}
        lower = int((want[3, 2][0] < want[0, 0][0]).sum())
        print("pairs strictly closer at (3, 2) than at (0, 0):", lower, "of 25; least clearance", want[0, 0][0].min(),
              want[3, 2][0].min(), want[pl.cap, pl.cap][0].min())
        assert lower > 0
        # clearance never grows when either slack grows
        for small, big in (((0, 0), (1, 0)), ((0, 0), (0, 1)), ((1, 0), (3, 2)), ((0, 1), (3, 2)), ((3, 2), (CH - 1, CH)),
                           ((1, 0), (CH + 1, 0)), ((CH - 1, CH), (pl.cap, pl.cap))):
            assert (want[big][0] <= want[small][0]).all(), (small, big)
    finally:
        pl.close()


def test_zero_slack_equals_the_cross_audit_bit_for_bit(pmaf, scenes, hip_lib):
    pl, scs, _ = rollout_case(pmaf, scenes, 2, T + 1, 2, 70, ragged=True)
    try:
        c0, s0 = pl.cross_audit(0, 1, SEP, step=True)
        c1, sa, sb = pl.cross_audit_slack(0, 1, SEP, 0, 0, steps=True)
        _same_bits(c1, c0, "slack (0, 0) against pmaf_cross_audit")
        np.testing.assert_array_equal(sa, s0)
        np.testing.assert_array_equal(sb, s0)
        paths, n = _paths(pl)
        c2, s2 = pl.cross_audit_tracks(0, paths[1], n[1], SEP, step=True)
        c3, ta, tb = pl.cross_audit_tracks_slack(0, paths[1], n[1], SEP, 0, 0, steps=True)
        _same_bits(c3, c2, "tracks, slack (0, 0) against pmaf_cross_audit_tracks")
        np.testing.assert_array_equal(ta, s2)
        np.testing.assert_array_equal(tb, s2)
    finally:
        pl.close()


@pytest.mark.parametrize("N,n_tracks", [(5, 3), (5, T + 1), (T + 1, 3)])
def test_tracks_variant(pmaf, scenes, hip_lib, N, n_tracks):
    """tracks of 0, 1, a middle number and cap points, n_tracks different from N"""
    pl, scs, _ = rollout_case(pmaf, scenes, 2, N, 2, CH + 6)
    try:
        paths, n = _paths(pl)
        cap = pl.cap
        rng = np.random.default_rng(5)
        tracks = rng.uniform(-1.0, 1.0, (n_tracks, cap, 3))
        tracks[:, :, 2] += 0.7
        ntp = np.asarray(([0, 1, cap // 2, cap] * n_tracks)[:n_tracks], dtype=np.int32)
        ntp[-1] = cap
        for t in range(n_tracks):
            tracks[t, ntp[t]:] = np.nan           # rows past the count are not read: a NaN there would be refused
        for late in slacks(cap):
            want = sref.cross_audit_slack(paths[1].tolist(), n[1].tolist(), tracks.tolist(), ntp.tolist(), SEP, late[0], late[1],
                                          hip_lib.pmaf_eval_order())
            got_c, got_a, got_b = pl.cross_audit_tracks_slack(1, tracks, ntp, SEP, late[0], late[1], steps=True)
            np.testing.assert_array_equal(got_a, np.asarray(want[1], dtype=np.int32), err_msg="step_a at %s" % (late,))
            np.testing.assert_array_equal(got_b, np.asarray(want[2], dtype=np.int32), err_msg="step_b at %s" % (late,))
            _same_bits(got_c, want[0], "clearance at %s" % (late,))
            _same_bits(pl.cross_audit_tracks_slack(1, tracks, ntp, SEP, late[0], late[1]), want[0], "clearance without steps")
            assert np.isinf(got_c[:, ntp == 0]).all() and (got_a[:, ntp == 0] == -1).all() and (got_b[:, ntp == 0] == -1).all()
    finally:
        pl.close()


def test_tracks_set_to_the_other_populations_paths(pmaf, scenes, hip_lib):
    pl, scs, _ = rollout_case(pmaf, scenes, 2, T + 1, 2, 70, ragged=True)
    try:
        paths, n = _paths(pl)
        for late in ((3, 2), (CH + 1, 0), (0, 2 * CH + 3), (pl.cap, pl.cap)):
            c0, a0, b0 = pl.cross_audit_slack(0, 1, SEP, late[0], late[1], steps=True)
            c1, a1, b1 = pl.cross_audit_tracks_slack(0, paths[1], n[1], SEP, late[0], late[1], steps=True)
            _same_bits(c1, c0, "tracks = population 1's paths at %s" % (late,))
            np.testing.assert_array_equal(a1, a0)
            np.testing.assert_array_equal(b1, b0)
    finally:
        pl.close()


def test_known_answers_at_rest(pmaf, scenes, hip_lib):
    """agents at rest at the origin against the walk of tests/test_cross_audit_gpu.py (x = 0.25 (4 - k), 7 and 3 points):
    d2 depends on the track's step alone, every admitted step of the agents ties and the smallest wins
    (tests/test_slack_audit.py derives the numbers). Two resting populations: every admitted pair ties: (0, 0)."""
    pl, scs = rest_pair(pmaf, scenes, [[0.0, 0.0, 0.0], [0.375, 0.5, 0.0]], 3)
    try:
        walk = np.zeros((2, pl.cap, 3))
        walk[:, :7, 0] = 0.25 * (4 - np.arange(7))
        for late_a in (0, 1, 5):
            for late_b in (0, 3):
                c, sa, sb = pl.cross_audit_tracks_slack(0, walk, [7, 3], 0.125, late_a, late_b, steps=True)
                print("slack", (late_a, late_b), c[0].tolist(), sa[0].tolist(), sb[0].tolist())
                assert (c[:, 0] == -0.125).all() and (sb[:, 0] == 4).all() and (sa[:, 0] == max(0, 4 - late_a)).all()
                assert (c[:, 1] == 0.375).all() and (sb[:, 1] == 2).all() and (sa[:, 1] == max(0, 2 - late_a)).all()
        for late in slacks(pl.cap):
            c, sa, sb = pl.cross_audit_slack(0, 1, 0.125, late[0], late[1], steps=True)
            assert (c == 0.5).all() and (sa == 0).all() and (sb == 0).all(), late
            c, sa, sb = pl.cross_audit_slack(1, 0, 1.0, late[0], late[1], steps=True)
            assert (c == -0.375).all() and (sa == 0).all() and (sb == 0).all(), late      # no floor
        check_slacked(pl, 0, 1, (3, 2), hip_lib, 0.125)
    finally:
        pl.close()


def test_nan_path_points_never_win(pmaf, scenes, hip_lib):
    """population 0: Had agents heading straight at an obstacle centred on the start-goal line latch a NaN rotation
    vector (the construction of tests/test_cross_audit_gpu.py): the paths turn NaN from there on and those steps never
    win, as either set, at slack (3, 2)"""
    scs = []
    for p in range(2):
        sc = scenes.synthetic_scene(3, 60, 1, 9, 2)
        sc["start"] = np.array([-0.44, 0.0 if p == 0 else 0.3, 0.7])
        sc["goal"] = np.array([0.6, 0.0 if p == 0 else 0.3, 0.7])
        sc["obstacles"][0] = [0.0, 0.0, 0.7, 0, 0, 0, 0.05]
        sc["agent_types"] = np.full(3, 6, dtype=np.int32)
        scs.append(sc)
    starts = np.stack([s["start"] for s in scs])
    pl = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    try:
        pl.set_initial_position(starts)
        pl.rollout()
        paths, n = _paths(pl)
        nan_pts = np.asarray([[int(np.isnan(paths[p, a, :n[p, a]]).any(axis=-1).sum()) for a in range(3)] for p in range(2)])
        print("NaN path points", nan_pts.tolist(), "of", n.tolist())
        assert nan_pts[0].min() > 0 and (nan_pts[0] < n[0]).all() and (nan_pts[1] == 0).all()
        c, sa, sb = check_slacked(pl, 0, 1, (3, 2), hip_lib)
        assert np.isfinite(c).all() and (sa < (n[0] - nan_pts[0])[:, None]).all()
        c, sa, sb = check_slacked(pl, 1, 0, (3, 2), hip_lib)
        assert np.isfinite(c).all() and (sb < (n[0] - nan_pts[0])[None, :]).all()
    finally:
        pl.close()


def test_select_pair_slack_against_the_reference(pmaf, scenes, hip_lib):
    pl, arms, starts = coupled_handle(pmaf, scenes, T + 1, 60)
    try:
        sc = arms[0]
        pl.rollout()
        pl.evaluate(sc["cost_gains"], sc["ws_limits"])
        costs = np.asarray(pl.costs())
        late = (3, 2)
        want_c, want_a, want_b = check_slacked(pl, 0, 1, late, hip_lib)
        plain_c, _ = ref.cross_audit(*[v for p in (0, 1) for v in (_paths(pl)[0][p].tolist(), _paths(pl)[1][p].tolist())], SEP,
                                     hip_lib.pmaf_eval_order())
        assert (want_c < np.asarray(plain_c)).any(), "the slacked matrix was meant to differ from the step-against-step one"
        margin = float(np.median(want_c))                   # from the REFERENCE's matrix: feasible for about half
        assert (want_c >= margin).any() and (want_c < margin).any()
        for m in (margin, float(want_c.max()) + 0.5):       # a feasible margin, an infeasible one
            pair, cost, clr, feas = ref.select_pair(want_c.tolist(), costs[0].tolist(), costs[1].tolist(), m)
            got = pl.select_pair_slack(0, 1, SEP, m, late[0], late[1])
            print("margin", m, "reference", pair, cost, clr, feas, "got", got)
            assert got["pair"] == pair and got["feasible"] == bool(feas)
            _same_bits(np.asarray([got["cost"], got["clearance"]]), [cost, clr], "pair cost / clearance")
            assert got["steps"] == (int(want_a[pair]), int(want_b[pair]))
        assert pl.select_pair_slack(0, 1, SEP, margin, late[0], late[1])["feasible"]
        assert not pl.select_pair_slack(0, 1, SEP, float(want_c.max()) + 0.5, late[0], late[1])["feasible"]
        # pair_steps may be NULL; (0, 0) is pmaf_select_pair
        pair = np.zeros(2, dtype=np.int32)
        cost, clr, feas = C.c_double(0), C.c_double(0), C.c_int32(0)
        ip = C.POINTER(C.c_int32)
        assert hip_lib.pmaf_select_pair_slack(pl._h, 0, 1, SEP, margin, 0, 0, pair.ctypes.data_as(ip), C.byref(cost),
                                              C.byref(clr), C.byref(feas), None) == 0
        plain = pl.select_pair(0, 1, SEP, margin)
        assert (int(pair[0]), int(pair[1])) == plain["pair"] and bool(feas.value) == plain["feasible"]
        _same_bits(np.asarray([cost.value, clr.value]), [plain["cost"], plain["clearance"]], "slack (0, 0) against pmaf_select_pair")
    finally:
        pl.close()


def test_calls_of_every_kind_share_one_handles_scratch(pmaf, scenes, hip_lib):
    """the six calls lay ONE grow-only scratch out per call (clearance | partials | result | tracks | step | track lengths
    | second step matrix): on one handle, 3 tracks, then a slacked population audit (the second step matrix appears), then
    T + 1 tracks slacked (the scratch grows and the second step matrix moves), a slacked pick, the plain audit, the plain
    pick, and the first call again -- every output of every call against the two references at tolerance 0, the last
    call's bits the first call's. Two chunks of steps, the second ragged."""
    pl, arms, starts = coupled_handle(pmaf, scenes, 5, CH + 6)
    try:
        sc, order = arms[0], hip_lib.pmaf_eval_order()
        pl.rollout()
        pl.evaluate(sc["cost_gains"], sc["ws_limits"])
        costs = np.asarray(pl.costs())
        paths, n = _paths(pl)
        cap = pl.cap
        assert CH < cap < 2 * CH, "the horizon was meant to give a second, ragged chunk"
        pop = [(paths[p].tolist(), n[p].tolist()) for p in (0, 1)]
        rng = np.random.default_rng(11)

        def make_tracks(n_tracks):
            tracks = rng.uniform(-1.0, 1.0, (n_tracks, cap, 3))
            tracks[:, :, 2] += 0.7
            ntp = np.asarray(([cap, 0, cap // 2, 1] * n_tracks)[:n_tracks], dtype=np.int32)
            for t in range(n_tracks):
                tracks[t, ntp[t]:] = np.nan       # rows past the count are not read
            return tracks, ntp

        def same(got, want, what):
            _same_bits(got[0], want[0], what + ": clearance")
            for g, w, name in zip(got[1:], want[1:], ("step_a", "step_b")):
                np.testing.assert_array_equal(g, np.asarray(w, dtype=np.int32), err_msg="%s: %s" % (what, name))

        def same_pick(got, matrix, margin, what):
            pair, cost, clr, feas = ref.select_pair(np.asarray(matrix).tolist(), costs[0].tolist(), costs[1].tolist(), margin)
            assert got["pair"] == pair and got["feasible"] == bool(feas), (what, got, pair, feas)
            _same_bits(np.asarray([got["cost"], got["clearance"]]), [cost, clr], what + ": pair cost / clearance")
            return pair

        few, n_few = make_tracks(3)
        many, n_many = make_tracks(T + 1)
        # 1. three tracks, step against step
        first = pl.cross_audit_tracks(0, few, n_few, SEP, step=True)
        want_first = ref.cross_audit(*pop[0], few.tolist(), n_few.tolist(), SEP, order)
        same(first, want_first, "1. cross_audit_tracks")
        # 2. the two populations, slacked, both step matrices
        same(pl.cross_audit_slack(0, 1, SEP, 2, 1, steps=True), sref.cross_audit_slack(*pop[0], *pop[1], SEP, 2, 1, order),
             "2. cross_audit_slack")
        # 3. T + 1 tracks, slacked: a larger scratch, every part behind the matrix at another offset
        same(pl.cross_audit_tracks_slack(1, many, n_many, SEP, 2, 1, steps=True),
             sref.cross_audit_slack(*pop[1], many.tolist(), n_many.tolist(), SEP, 2, 1, order), "3. cross_audit_tracks_slack")
        # 4. the slacked pick
        want = sref.cross_audit_slack(*pop[0], *pop[1], SEP, 3, 2, order)
        got = pl.select_pair_slack(0, 1, SEP, float(np.median(want[0])), 3, 2)
        pair = same_pick(got, want[0], float(np.median(want[0])), "4. select_pair_slack")
        assert got["steps"] == (int(np.asarray(want[1])[pair]), int(np.asarray(want[2])[pair]))
        # 5. the plain audit, 6. the plain pick
        want = ref.cross_audit(*pop[0], *pop[1], SEP, order)
        same(pl.cross_audit(0, 1, SEP, step=True), want, "5. cross_audit")
        same_pick(pl.select_pair(0, 1, SEP, float(np.median(want[0]))), want[0], float(np.median(want[0])), "6. select_pair")
        # 7. the first call again
        again = pl.cross_audit_tracks(0, few, n_few, SEP, step=True)
        same(again, want_first, "7. cross_audit_tracks again")
        _same_bits(again[0], first[0], "the first call's clearance")
        np.testing.assert_array_equal(again[1], first[1])
    finally:
        pl.close()


def _tick_run(pmaf, scenes, late, audit, n_ticks=4):
    pl, arms, starts = coupled_handle(pmaf, scenes, 5, 30)
    try:
        sc = arms[0]
        cpl = pmaf.shard.DualArmCoupling(np.stack([s["obstacles"] for s in arms]), 0.1)
        pl.start()
        rec = []
        for t in range(n_ticks):
            if audit:
                pl.stop()
                paths, n = _paths(pl)
                pl.cross_audit_slack(0, 1, SEP, 3, 2, steps=(t % 2 == 0))
                pl.cross_audit_tracks_slack(1, paths[0], n[0], SEP, 2, CH + 1, steps=(t % 2 == 1))
                pl.select_pair_slack(0, 1, SEP, 0.05, 10 ** 6, 0)
            kw = {} if late == "default" else {"late": late}
            out = cpl.pair_tick(pl, sc["dt"], sc["cost_gains"], sc["ws_limits"], margin=0.02, agent_radius=sc["radius"], **kw)
            pl.stop()
            rec.append((out, _results(pl)))
        return rec, starts
    finally:
        pl.close()


def _assert_same_runs(r0, r1):
    for (o0, g0), (o1, g1) in zip(r0, r1):
        assert o0["pair"] == o1["pair"] and o0["feasible"] == o1["feasible"]
        assert len(g0) == len(g1)
        for i, (x, y) in enumerate(zip(g0, g1)):
            if x.dtype.kind == "f":
                _same_bits(y, x, "getter %d" % i)
            else:
                np.testing.assert_array_equal(y, x, err_msg="getter %d" % i)


def test_pair_tick_with_slack(pmaf, scenes, hip_lib):
    """late=(3, 2): coupled ticks through pmaf_select_pair_slack; late=None: bit-identical to a call without the
    argument; late=(0, 0): the same pairs as the un-slacked pick (another kernel, the same matrix)"""
    slack, starts = _tick_run(pmaf, scenes, (3, 2), False)
    for out, getters in slack:
        assert 0 <= out["pair"][0] < 5 and 0 <= out["pair"][1] < 5 and np.isfinite(out["positions"]).all()
        sa, sb = out["steps"]
        assert sa >= 0 and sb >= 0 and sb - sa <= 3 and sa - sb <= 2
    assert (np.abs(slack[-1][0]["positions"] - starts) > 0).any(), "the arms were meant to move"
    default, _ = _tick_run(pmaf, scenes, "default", False)
    none, _ = _tick_run(pmaf, scenes, None, False)
    assert all("steps" not in out for out, _ in none)
    _assert_same_runs(default, none)
    zero, _ = _tick_run(pmaf, scenes, (0, 0), False)
    _assert_same_runs(default, zero)


def test_the_three_calls_change_no_state(pmaf, scenes, hip_lib):
    """the same tick sequence with and without the three new calls in between: every result getter bit-identical"""
    without, _ = _tick_run(pmaf, scenes, None, False)
    with_calls, _ = _tick_run(pmaf, scenes, None, True)
    _assert_same_runs(without, with_calls)


def test_error_paths(pmaf, scenes, hip_lib):
    pl, arms, starts = coupled_handle(pmaf, scenes, 4, 10)
    try:
        L, h = hip_lib, pl._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        N, cap = 4, pl.cap
        clr, sa, sb = np.zeros((N, N)), np.zeros((N, N), dtype=np.int32), np.zeros((N, N), dtype=np.int32)
        c_p, a_p, b_p = clr.ctypes.data_as(dp), sa.ctypes.data_as(ip), sb.ctypes.data_as(ip)
        pair, st = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        cost, pc, fe = C.c_double(0), C.c_double(0), C.c_int32(0)
        sel = (pair.ctypes.data_as(ip), C.byref(cost), C.byref(pc), C.byref(fe), st.ctypes.data_as(ip))
        pl.rollout()
        tr = np.zeros((3, cap, 3))
        ntp = np.asarray([cap, 2, 0], dtype=np.int32)
        t_p, n_p = tr.ctypes.data_as(dp), ntp.ctypes.data_as(ip)
        assert L.pmaf_cross_audit_slack(h, 0, 1, SEP, 1, 1, c_p, a_p, b_p) == 0
        assert L.pmaf_cross_audit_tracks_slack(h, 0, 3, t_p, n_p, SEP, 1, 1, c_p, a_p, b_p) == 0
        for la, lb in ((-1, 0), (0, -1), (-5, -5), (-2 ** 31, 3)):                        # negative slack
            assert L.pmaf_cross_audit_slack(h, 0, 1, SEP, la, lb, c_p, a_p, b_p) == -1, (la, lb)
            assert b"late" in L.pmaf_last_error()
            assert L.pmaf_cross_audit_tracks_slack(h, 0, 3, t_p, n_p, SEP, la, lb, c_p, a_p, b_p) == -1, (la, lb)
            assert L.pmaf_select_pair_slack(h, 0, 1, SEP, 0.0, la, lb, *sel) == -1, (la, lb)
        assert L.pmaf_cross_audit_slack(h, 0, 1, SEP, 2 ** 31 - 1, 2 ** 31 - 1, c_p, a_p, b_p) == 0    # clamped, not overflowed
        for a, b in ((0, 0), (1, 1), (-1, 0), (0, 2), (2, 0), (0, -1)):                   # equal or out-of-range populations
            assert L.pmaf_cross_audit_slack(h, a, b, SEP, 1, 1, c_p, a_p, b_p) == -1, (a, b)
            assert L.pmaf_select_pair_slack(h, a, b, SEP, 0.0, 1, 1, *sel) == -1, (a, b)
        assert L.pmaf_cross_audit_slack(h, 0, 1, SEP, 1, 1, None, a_p, b_p) == -1         # NULL clearance
        assert L.pmaf_cross_audit_slack(None, 0, 1, SEP, 1, 1, c_p, a_p, b_p) == -1
        assert L.pmaf_cross_audit_slack(h, 0, 1, float("nan"), 1, 1, c_p, a_p, b_p) == -1
        assert L.pmaf_cross_audit_slack(h, 0, 1, SEP, 1, 1, c_p, None, b_p) == 0          # either step pointer alone
        assert L.pmaf_cross_audit_slack(h, 0, 1, SEP, 1, 1, c_p, a_p, None) == 0
        for k in range(4):
            args = list(sel)
            args[k] = None
            assert L.pmaf_select_pair_slack(h, 0, 1, SEP, 0.0, 1, 1, *args) == -1, k
        assert L.pmaf_select_pair_slack(h, 0, 1, SEP, float("inf"), 1, 1, *sel) == -1
        for n_tracks in (0, -1):                                                          # n_tracks <= 0
            assert L.pmaf_cross_audit_tracks_slack(h, 0, n_tracks, t_p, n_p, SEP, 1, 1, c_p, a_p, b_p) == -1
        for bad in (cap + 1, -1):                                                         # a count outside [0, cap]
            ntp[1] = bad
            assert L.pmaf_cross_audit_tracks_slack(h, 0, 3, t_p, n_p, SEP, 1, 1, c_p, a_p, b_p) == -1, bad
        ntp[1] = 2
        assert L.pmaf_cross_audit_tracks_slack(h, 2, 3, t_p, n_p, SEP, 1, 1, c_p, a_p, b_p) == -1
        assert L.pmaf_cross_audit_tracks_slack(h, 0, 3, None, n_p, SEP, 1, 1, c_p, a_p, b_p) == -1
        assert L.pmaf_cross_audit_tracks_slack(h, 0, 3, t_p, None, SEP, 1, 1, c_p, a_p, b_p) == -1
        assert L.pmaf_cross_audit_tracks_slack(h, 0, 3, t_p, n_p, SEP, 1, 1, None, a_p, b_p) == -1
        tr[1, 1, 2] = np.inf                                                              # inside the count: range-checked
        assert L.pmaf_cross_audit_tracks_slack(h, 0, 3, t_p, n_p, SEP, 1, 1, c_p, a_p, b_p) == -1
        assert b"range" in L.pmaf_last_error()
        tr[1, 1, 2] = 0.0
        tr[1, 2, 2] = np.inf                                                              # past the count: not read
        assert L.pmaf_cross_audit_tracks_slack(h, 0, 3, t_p, n_p, SEP, 1, 1, c_p, None, None) == 0
        # the handle is still usable, and still right
        check_slacked(pl, 0, 1, (3, 2), hip_lib)
        pl.evaluate(arms[0]["cost_gains"], arms[0]["ws_limits"])
        assert pl.select_pair_slack(0, 1, SEP, -1.0, 3, 2)["feasible"]
    finally:
        pl.close()
