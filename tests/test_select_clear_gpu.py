"""Selection against the live list on the GPU (pmaf_select_clear / pmaf_adopt_best, include/pmaf.h) through the C-ABI
against tests/select_clear_reference.py at TOLERANCE 0: integers equal, doubles bit-equal, a NaN matched by a NaN. The
reference is fed the handle's own paths(), costs() and the live list, and takes its dot association from
pmaf_eval_order(), so the file passes unchanged under PMAF_VARIANT=rassoc. Scenes are built as in
tests/test_path_audit_gpu.py (its rollout_case, live_list and rest_planner); every select call comes after one
pmaf_evaluate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conftest
import select_clear_reference as ref
from test_path_audit_gpu import live_list, rest_planner, rollout_case

pytestmark = pytest.mark.gpu

ROOT = conftest.ROOT
INT_KEYS = ("pick", "rule", "n_clear", "first_violation")
DBL_KEYS = ("cost", "clearance")


def _same_bits(got, want, what):
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float64).reshape(-1))
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float64).reshape(-1))
    assert got.shape == want.shape, what
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), "%s: %d of %d values differ, first at %s: %r != %r" % (
        what, (~ok).sum(), ok.size, np.argwhere(~ok)[0], got[~ok][0], want[~ok][0])


def _evaluate(pl, sc):
    return pl.evaluate(sc["cost_gains"], sc["ws_limits"])


def _handle_tables(pl):
    """the handle's own paths, lengths and costs as [P][N]... lists"""
    paths, n = pl.paths()
    paths = np.asarray(paths).reshape(pl.P, pl.N, pl.cap, 3)
    n = np.asarray(n).reshape(pl.P, pl.N)
    costs = np.asarray(pl.costs()).reshape(pl.P, pl.N)
    return paths.tolist(), n.tolist(), costs.tolist()


def check_select(pl, sc, obs, margin, horizon, hip_lib, prev=None, tables=None, what="", audits=None):
    """one pmaf_select_clear call (adopt = 0) compared with the reference on the handle's own tables; returns the call's
    dict with every value as an array over the populations"""
    obs = np.asarray(obs, dtype=np.float64).reshape(pl.P, pl.n_obs, 7)
    got = pl.select_clear(obs, margin, horizon, prev=prev)
    got = {k: np.asarray(v).reshape(pl.P) for k, v in got.items()}
    paths, n, costs = tables if tables is not None else _handle_tables(pl)
    pv = None if prev is None else np.broadcast_to(np.asarray(prev), (pl.P,)).tolist()
    audited = None
    if audits is not None:   # the reference's window audit of (margin, horizon), computed once and shared
        if (margin, horizon) not in audits:
            audits[(margin, horizon)] = ref.window_audit(paths, n, obs.tolist(), sc["dt"], sc.get("radius", 0.05), margin,
                                                         horizon, hip_lib.pmaf_eval_order())
        audited = audits[(margin, horizon)]
    want = ref.select_clear(paths, n, obs.tolist(), costs, sc["dt"], sc.get("radius", 0.05), margin, horizon,
                            hip_lib.pmaf_eval_order(), pv, audited)
    tag = "%s margin %r horizon %r prev %r" % (what, margin, horizon, prev)
    print(tag, "got", {k: v.tolist() for k, v in got.items()})
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], np.asarray(want[k]), err_msg=k + " " + tag)
    for k in DBL_KEYS:
        _same_bits(got[k], want[k], k + " " + tag)
    assert ((got["pick"] >= 0) & (got["pick"] < pl.N)).all()
    return got


# (P, N, M, H, ragged): 1, 3, 32 and 67 obstacles bracket one 64-lane obstacle tile; 65 and 130 agents make the pick
# stride past one wave of agents; the ragged case has paths of different lengths
SHAPES = [(2, 5, 2, 8, False), (2, 5, 66, 70, False), (1, 5, 66, 8, False), (1, 5, 31, 70, False), (1, 1, 0, 8, False),
          (2, 5, 2, 70, True), (1, 65, 2, 8, False), (1, 130, 2, 8, False)]
# margins: all clear / none clear everywhere, and three in between that cut through the clearances of the H = 70 shapes
# (0.062 .. 0.094, 0.089 .. 0.106, 0.145 .. 0.159 at the full horizon; short windows see identical path starts)
MARGINS = (-0.5, 0.075, 0.092, 0.155, 3.0)
_SEEN = {}


def _run_shape(pmaf, scenes, hip_lib, shape):
    """every horizon x margin of one shape, without and with a previous pick; returns the (rule, n_clear regime) pairs
    seen. Run once per shape and session."""
    if shape in _SEEN:
        return _SEEN[shape]
    P, N, M, H, ragged = shape
    pl, scs, start = rollout_case(pmaf, scenes, P, N, M, H, ragged)
    seen = set()
    try:
        _evaluate(pl, scs[0])
        live = live_list(scenes, start)
        tables = _handle_tables(pl)
        audits = {}
        for hi, horizon in enumerate((1, 3, H // 2, H + 1, H + 6)):
            for mi, margin in enumerate(MARGINS):
                for prev in (None, [(hi + mi + p) % N for p in range(P)]):
                    got = check_select(pl, scs[0], live, margin, horizon, hip_lib, prev, tables, str(shape), audits)
                    for p in range(P):
                        nc = int(got["n_clear"][p])
                        seen.add((int(got["rule"][p]), 0 if nc == 0 else (2 if nc == N else 1)))
    finally:
        pl.close()
    _SEEN[shape] = seen
    return seen


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "P%d-N%d-M%d-H%d%s" % (s[0], s[1], s[2], s[3], "-ragged" if s[4] else ""))
def test_shapes_horizons_margins(pmaf, scenes, hip_lib, shape):
    seen = _run_shape(pmaf, scenes, hip_lib, shape)
    print("(rule, n_clear regime) seen:", sorted(seen))
    assert seen


@pytest.mark.parametrize("horizon", [1, 2, 3, 5])
def test_windows_shorter_than_two_points_per_wave(pmaf, scenes, hip_lib, horizon):
    """the audit splits the window of w = min(n, horizon) points over four waves in quarters of ceil(w / 4): w = 1, 2, 3
    leave waves without a step (k0 == k1), w = 5 gives quarters of 2, 2, 1, 0 -- at P = 2, N = 5, M = 3, 9 points"""
    pl, scs, start = rollout_case(pmaf, scenes, 2, 5, 3, 8)
    try:
        _evaluate(pl, scs[0])
        live = live_list(scenes, start)
        tables, audits = _handle_tables(pl), {}
        assert all(n >= 5 for row in tables[1] for n in row)      # w = horizon for every agent
        for margin in MARGINS:
            got = check_select(pl, scs[0], live, margin, horizon, hip_lib, [1, 3], tables, "short window", audits)
            assert (got["first_violation"] <= horizon).all()
    finally:
        pl.close()


def test_every_rule_and_every_n_clear_regime_occurred(pmaf, scenes, hip_lib):
    seen = set()
    for shape in SHAPES:
        seen |= _run_shape(pmaf, scenes, hip_lib, shape)
    print("(rule, n_clear regime) over the whole parametrisation:", sorted(seen))
    assert {r for r, _ in seen} == {0, 1, 2}
    assert {g for _, g in seen} == {0, 1, 2}     # no agent clear, some, all


def test_every_previous_pick_in_turn(pmaf, scenes, hip_lib):
    pl, scs, start = rollout_case(pmaf, scenes, 2, 5, 2, 8)
    try:
        _evaluate(pl, scs[0])
        live = live_list(scenes, start)
        tables = _handle_tables(pl)
        audits = {}
        for margin in (-0.5, 0.3, 3.0):
            none = check_select(pl, scs[0], live, margin, 9, hip_lib, None, tables, audits=audits)
            minus = check_select(pl, scs[0], live, margin, 9, hip_lib, -1, tables, audits=audits)
            for k in INT_KEYS + DBL_KEYS:
                _same_bits(np.asarray(minus[k], dtype=np.float64), np.asarray(none[k], dtype=np.float64), k)
            for q in range(5):
                check_select(pl, scs[0], live, margin, 9, hip_lib, q, tables, audits=audits)
                check_select(pl, scs[0], live, margin, 9, hip_lib, [q, (q + 2) % 5], tables, audits=audits)
    finally:
        pl.close()


def test_hand_derived_moving_obstacle(pmaf, scenes, hip_lib):
    """test_path_audit_gpu.test_hand_derived_moving_obstacle's geometry: c(k) = 0.625 - 0.0625 k. Literal expectations."""
    moving = [[1.0, 0.0, 0.0, -0.5, 0.0, 0.0, 0.25]]
    pl, sc = rest_planner(pmaf, scenes, moving, [0.0, 0.0, 0.0])
    try:
        _evaluate(pl, sc)
        cost = float(np.asarray(pl.costs()).reshape(-1)[0])
        assert cost < float("inf")               # (rule 1 needs a comparable cost)
        r = pl.select_clear(moving, 0.45, 3)
        print("cost", cost, "horizon 3", r)
        assert (r["pick"], r["rule"], r["n_clear"], r["first_violation"], r["clearance"]) == (0, 1, 1, 3, 0.5)
        _same_bits([r["cost"]], [cost], "the pick's cost")
        r = pl.select_clear(moving, 0.45, 4)
        print("horizon 4", r)
        assert (r["pick"], r["rule"], r["n_clear"], r["first_violation"], r["clearance"]) == (0, 2, 0, 3, 0.4375)
        r = pl.select_clear(moving, 0.2, 1000)   # above the cap: the whole path of 7 points
        assert (r["n_clear"], r["first_violation"], r["clearance"]) == (1, 7, 0.25)
    finally:
        pl.close()


def test_cost_tie_goes_to_the_smaller_index(pmaf, scenes, hip_lib):
    """identical agents (same type, same gains) have identical paths and costs"""
    sc = scenes.synthetic_scene(4, 20, 3, config_id=7, dynamic=True, agent_types=[1, 1, 1, 1])
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        pl.rollout()
        _evaluate(pl, sc)
        costs = np.asarray(pl.costs())
        assert np.isfinite(costs).all() and (costs == costs[0]).all(), costs
        live = scenes.advance_live_obstacles(sc["obstacles"])
        got = check_select(pl, sc, live, -0.5, 21, hip_lib)
        assert (int(got["pick"][0]), int(got["rule"][0]), int(got["n_clear"][0])) == (0, 1, 4)
        got = check_select(pl, sc, live, -0.5, 21, hip_lib, prev=2)      # cost[m] >= 0.9 * cost[q]: q is kept
        assert (int(got["pick"][0]), int(got["rule"][0])) == (2, 0)
        got = check_select(pl, sc, live, 3.0, 21, hip_lib, prev=2)       # nobody clear: the fallback ties to index 0
        assert (int(got["pick"][0]), int(got["rule"][0]), int(got["n_clear"][0])) == (0, 2, 0)
    finally:
        pl.close()


def test_nan_paths_never_become_the_pick(pmaf, scenes, hip_lib):
    """the Had scene of test_path_audit_gpu.test_nan_path_points_never_win with one Goal-heuristic agent beside the two
    Had agents whose paths (and costs) turn NaN. Wherever an agent is clear the pick is the agent with the finite cost.
    With nobody clear (margin 10) the contract's rule 2 orders by first violation, clearance and index and does not look
    at costs: there the pick is agent 0, a NaN agent (fv 0 for all three, c 0.3265 the greatest), as the reference says."""
    sc = scenes.synthetic_scene(3, 60, 1, 9, 2)
    sc["start"] = np.array([-0.44, 0.0, 0.7])
    sc["goal"] = np.array([0.6, 0.0, 0.7])
    sc["obstacles"][0] = [0.0, 0.0, 0.7, 0, 0, 0, 0.05]
    sc["agent_types"] = np.array([6, 1, 6], dtype=np.int32)
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        pl.rollout()
        _evaluate(pl, sc)
        paths, n = pl.paths()
        costs = np.asarray(pl.costs())
        nan_agent = [bool(np.isnan(paths[a, :n[a]]).any()) for a in range(3)]
        print("NaN path per agent", nan_agent, "costs", costs.tolist())
        assert nan_agent == [True, False, True] and np.isfinite(costs[1])
        # wherever an agent is clear the pick has a comparable cost: never a NaN agent (agent 1's cost is finite)
        for margin in (-0.5, 0.01):
            for horizon in (5, 30, 61):
                for prev in (None, 0, 1, 2):
                    got = check_select(pl, sc, sc["obstacles"], margin, horizon, hip_lib, prev)
                    assert int(got["pick"][0]) == 1 and int(got["rule"][0]) in (0, 1), (margin, horizon, prev)
        # nobody clear: rule 2 orders by fv, then c, then index and does not look at costs (include/pmaf.h), so it may
        # name a NaN agent; held to the reference only
        for prev in (None, 1):
            got = check_select(pl, sc, sc["obstacles"], 10.0, 61, hip_lib, prev)
            assert int(got["rule"][0]) == 2 and int(got["n_clear"][0]) == 0
    finally:
        pl.close()


def test_argument_validation(pmaf, scenes, hip_lib):
    sc = scenes.synthetic_scene(4, 10, 3, config_id=7)
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        pl.rollout()
        _evaluate(pl, sc)
        L, h = hip_lib, pl._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        obs = np.ascontiguousarray(sc["obstacles"], dtype=np.float64)
        o_p = obs.ctypes.data_as(dp)
        outs_i = [np.full(1, -7, dtype=np.int32) for _ in range(4)]     # pick, rule, n_clear, first_violation
        outs_d = [np.full(1, -7.0) for _ in range(2)]                   # cost, clearance

        def call(h_, o_, margin, horizon, prev, adopt, mask=0x3f):
            a = [x.ctypes.data_as(ip) for x in outs_i]
            d = [x.ctypes.data_as(dp) for x in outs_d]
            args = [a[0], a[1], a[2], d[0], d[1], a[3]]
            args = [v if mask >> i & 1 else None for i, v in enumerate(args)]
            return L.pmaf_select_clear(h_, o_, margin, horizon, prev, adopt, *args)

        assert call(None, o_p, 0.05, 5, None, 0) == -1
        assert call(h, None, 0.05, 5, None, 0) == -1
        assert call(h, o_p, 0.05, 5, None, 0, mask=0x3e) == -1           # pick is required
        assert L.pmaf_adopt_best(None, outs_i[0].ctypes.data_as(ip)) == -1 and L.pmaf_adopt_best(h, None) == -1
        for horizon in (0, -1, -2 ** 31):
            assert call(h, o_p, 0.05, horizon, None, 0) == -1, horizon
        for bad_prev in (4, -2):
            pv = np.array([bad_prev], dtype=np.int32)
            assert call(h, o_p, 0.05, 5, pv.ctypes.data_as(ip), 0) == -1, bad_prev
            assert L.pmaf_adopt_best(h, pv.ctypes.data_as(ip)) == -1, bad_prev
        assert call(h, o_p, float("nan"), 5, None, 0) == -1
        bad = obs.copy()
        bad[1, 4] = np.nan
        assert call(h, bad.ctypes.data_as(dp), 0.05, 5, None, 0) == -1
        assert b"range" in L.pmaf_last_error()
        assert pl.best()[1][0] > 0 and all(int(x[0]) == -7 for x in outs_i)   # nothing written, nothing adopted
        # every optional output NULL in turn: the others unchanged
        assert call(h, o_p, 0.05, 5, None, 0) == 0
        full_i, full_d = [x.copy() for x in outs_i], [x.copy() for x in outs_d]
        order = [("i", 0), ("i", 1), ("i", 2), ("d", 0), ("d", 1), ("i", 3)]
        for drop in range(1, 6):
            for x in outs_i:
                x[:] = -7
            for x in outs_d:
                x[:] = -7.0
            assert call(h, o_p, 0.05, 5, None, 0, mask=0x3f & ~(1 << drop)) == 0
            for i, (kind, k) in enumerate(order):
                got = (outs_i if kind == "i" else outs_d)[k]
                want = (full_i if kind == "i" else full_d)[k]
                if i == drop:
                    assert got[0] == -7
                elif kind == "i":
                    np.testing.assert_array_equal(got, want)
                else:
                    _same_bits(got, want, "optional output %d" % i)
    finally:
        pl.close()


def test_refused_after_an_abandoned_tick(pmaf, scenes, hip_lib, monkeypatch):
    """a tick that ran into its time limit (test_failure_detection_gpu's fault injection: the sequence number withheld
    while a long rollout keeps the stream busy) leaves the handle abandoned until pmaf_stop: both calls refuse it"""
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
            pl.select_clear(sc["obstacles"], 0.05, 5)
        assert e.value.code == -3, str(e.value)
        with pytest.raises(pmaf.PmafError) as e:
            pl.adopt_best(0)
        assert e.value.code == -3, str(e.value)
        pl.stop()
        r = pl.select_clear(sc["obstacles"], 0.05, 5)
        assert 0 <= r["pick"] < 512
        pl.adopt_best(r["pick"])
        assert pl.best_id() == r["pick"] + 1
    finally:
        pl.close()


def test_a_select_without_adoption_between_ticks_changes_nothing(pmaf, scenes, hip_lib):
    """best indices and set-points of 5 ticks on C1 with moving lists, with and without select calls in between:
    bit-identical. The select call is given the list of the FOLLOWING tick: a call that wrongly marked its list as the
    resident live list would make that tick hand nothing over."""
    sc = scenes.config_scene("C1")
    lists = [sc["obstacles"]]
    for t in range(5):
        nxt = scenes.advance_live_obstacles(lists[-1])
        nxt[:-1, 3:6] = 0.02 * (t + 1)           # (the static scene's obstacles start to move)
        lists.append(nxt)
    runs = []
    for select in (False, True):
        pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
        try:
            pl.set_initial_position(sc["start"])
            rec = []
            for t in range(5):
                b = pl.tick(lists[t], sc["dt"], sc["cost_gains"], sc["ws_limits"])
                rec.append((int(b), pl.last_next_pos.copy(), pl.last_next_vel.copy()))
                if select:
                    r = pl.select_clear(lists[t + 1], 0.05, 50 if t % 2 else 1000, prev=None if t == 0 else int(b))
                    assert 0 <= r["pick"] < pl.N
            pl.stop()
            rec.append((0, np.asarray(pl.paths()[0]).copy(), np.asarray(pl.real_known()[1]).copy()))
            runs.append(rec)
        finally:
            pl.close()
    for (b0, p0, v0), (b1, p1, v1) in zip(*runs):
        assert b0 == b1
        _same_bits(p1, p0, "set-point position / paths")
        _same_bits(v1, v0, "set-point velocity / real rotation vectors")


def _ragged_gain_scenes(scenes, P, N, M, H):
    scs = []
    for p in range(P):
        sc = scenes.synthetic_scene(N, H, M, config_id=7, scene_id=p, dynamic=True)
        sc["k_attr"] = np.linspace(2.0, 6.0, N)         # different gains per agent: move_real's agent_id matters too
        sc["k_circ"] = np.linspace(0.02, 0.04, N)
        sc["k_damp"] = np.linspace(2.5, 4.0, N)
        scs.append(sc)
    return scs


def _state(pl):
    t, i = pl.best()
    pos, vel, force = pl.real_state()
    known, rot = pl.real_known()
    paths, n = pl.paths()
    return (np.asarray(t).copy(), np.asarray(i).copy(), np.asarray(n).copy(), np.asarray(known).copy(),
            [np.asarray(a).copy() for a in (pos, vel, force, rot, paths)])


def _same_state(a, b, what):
    for x, y, k in zip(a[:4], b[:4], ("best type", "best id", "n_points", "real known")):
        np.testing.assert_array_equal(x, y, err_msg=what + " " + k)
    for x, y, k in zip(a[4], b[4], ("real pos", "real vel", "real force", "real rot", "paths")):
        _same_bits(x, y, what + " " + k)


def _host_adopt(pl, scs, picks):
    """what pmaf_adopt_best does, the host way: pmaf_set_best with the Random vectors the caller kept; -1 = keep"""
    t, i = pl.best()
    layout = [6, 1, 2, 3, 4]   # pmaf_create's default types: Had, Goal, Obstacle, GoalObstacle, Vel, then Random (5)
    ids, types, rv = [], [], []
    for p, a in enumerate(np.broadcast_to(np.asarray(picks), (pl.P,)).tolist()):
        a = a if a >= 0 else int(i[p]) - 1
        assert a >= 0
        ids.append(a + 1)
        types.append(layout[a] if a < 5 else 5)
        rv.append(np.asarray(scs[p]["random_vecs"])[a])
    pl.set_best(ids, types, np.stack(rv))


def test_adoption_equals_the_host_path(pmaf, scenes, hip_lib):
    """two handles on the same scene, 6 ticks of the six-call sequence: A adopts on the device (adopt = 1), B selects
    with adopt = 0 and applies the pick through pmaf_set_best"""
    P, N, M, H = 2, 7, 5, 40
    scs = _ragged_gain_scenes(scenes, P, N, M, H)
    starts = np.stack([s["start"] for s in scs])
    obs = np.stack([s["obstacles"] for s in scs])
    sc = scs[0]
    A = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    B = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    try:
        for pl in (A, B):
            pl.set_initial_position(starts)
            pl.start()
        prev = None
        picks_seen = set()
        for t in range(6):
            live = live_list(scenes, obs)
            margin = (0.02, 0.06, 0.1)[t % 3]
            a = A.audited_tick(live, sc["dt"], sc["cost_gains"], sc["ws_limits"], margin, 30, prev=prev)
            B.stop()
            B.evaluate(sc["cost_gains"], sc["ws_limits"])
            b = B.select_clear(live, margin, 30, prev=prev, adopt=False)
            _host_adopt(B, scs, b["pick"])
            B.move_real(live, sc["dt"], 1, b["pick"])
            pos, vel, _ = B.real_state()
            B.reset_agents(pos, vel, live)
            B.start()
            print("tick", t, "A", {k: np.asarray(v).tolist() for k, v in a.items()})
            for k in INT_KEYS:
                np.testing.assert_array_equal(a[k], b[k], err_msg="tick %d %s" % (t, k))
            for k in DBL_KEYS:
                _same_bits(a[k], b[k], "tick %d %s" % (t, k))
            np.testing.assert_array_equal(A.best()[1], np.asarray(a["pick"]) + 1)
            _same_state(_state(A), _state(B), "tick %d" % t)
            prev = np.asarray(a["pick"]).copy()
            picks_seen.update(prev.tolist())
            obs = live
        print("picks seen", sorted(picks_seen))
    finally:
        A.close()
        B.close()


def test_adopt_best_alone_equals_set_best(pmaf, scenes, hip_lib):
    """pmaf_adopt_best against pmaf_set_best over 6 ticks, P = 2; an entry of -1 leaves its population untouched"""
    P, N, M, H = 2, 7, 5, 40
    scs = _ragged_gain_scenes(scenes, P, N, M, H)
    starts = np.stack([s["start"] for s in scs])
    obs = np.stack([s["obstacles"] for s in scs])
    sc = scs[0]
    A = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    B = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    try:
        for pl in (A, B):
            pl.set_initial_position(starts)
            pl.start()
        for t in range(6):
            picks = np.array([(3 * t + 1) % N, -1 if t % 2 == 0 else (t + 5) % N], dtype=np.int32)
            states = []
            for pl in (A, B):
                pl.stop()
                best = np.asarray(pl.evaluate(sc["cost_gains"], sc["ws_limits"]))
                before = pl.best()
                if pl is A:
                    pl.adopt_best(picks)
                else:
                    _host_adopt(pl, scs, picks)
                after = pl.best()
                for p in range(P):
                    if picks[p] < 0:
                        assert (after[0][p], after[1][p]) == (before[0][p], before[1][p])
                    else:
                        assert after[1][p] == picks[p] + 1
                ids = np.where(picks >= 0, picks, best).astype(np.int32)
                pl.move_real(obs, sc["dt"], 1, ids)
                pos, vel, _ = pl.real_state()
                pl.reset_agents(pos, vel, obs)
                pl.start()
                states.append(_state(pl))
            _same_state(states[0], states[1], "tick %d" % t)
            obs = live_list(scenes, obs)
    finally:
        A.close()
        B.close()


def _blocked_winner_case(pmaf, scenes):
    """Uniform gains. Field obstacle 0 sits just off the start-goal line, so the heuristics pass it on different sides;
    field obstacle 1 is far away. After 50 ticks the real agent is under way (its gate is open) and the live list (a)
    brings obstacle 1 into the real agent's shell -- first contact: the rotation vector the real step latches depends
    on the best agent's heuristic -- and (b) puts a small sphere on evaluate's winner's path. Returns the handle stopped
    right behind pmaf_evaluate, the scene, the live list and evaluate's best."""
    sc = scenes.synthetic_scene(12, 250, 2, config_id=7, scene_id=3)
    sc["obstacles"][0] = [-0.25, 0.02, 0.71, 0.0, 0.0, 0.0, 0.08]
    sc["obstacles"][1] = [0.0, 2.0, 0.7, 0.0, 0.0, 0.0, 0.02]
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    pl.set_initial_position(sc["start"])
    for _ in range(50):
        pl.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
    pl.stop()
    best = int(pl.evaluate(sc["cost_gains"], sc["ws_limits"]))
    paths, n = pl.paths()
    live = np.array(sc["obstacles"], copy=True)
    live[1, 0:3] = np.asarray(pl.real_state()[0]) + np.array([0.1, 0.15, 0.1])
    k = int(int(n[best]) * 0.7)
    live[-1] = [paths[best, k, 0], paths[best, k, 1], paths[best, k, 2], 0.0, 0.0, 0.0, 0.02]
    return pl, sc, live, best


def test_the_real_step_follows_the_pick_only_with_adoption(pmaf, scenes, hip_lib):
    """The reason the calls exist. evaluate's winner is blocked by the live list and a Random agent is clear. With
    uniform gains move_real(agent_id = pick) WITHOUT adoption gives the set-point of agent_id = evaluate's best, bit for
    bit: agent_id selects gains only. WITH adoption get_best reports the pick's type and the set-point differs."""
    setpoints = {}
    for mode in ("best", "pick", "adopted"):
        pl, sc, live, best = _blocked_winner_case(pmaf, scenes)
        try:
            types_before, ids_before = pl.best()
            sel = check_select(pl, sc, live, 0.03, 251, hip_lib, prev=best)
            pick = int(sel["pick"][0])
            print(mode, "evaluate's best", best, "type", int(types_before[0]), "select", {k: v.tolist() for k, v in sel.items()})
            assert 0 < int(sel["n_clear"][0]) < pl.N and int(sel["rule"][0]) == 1
            assert pick != best and pick >= 5, "the scene is meant to block the winner and leave a Random agent clear"
            assert int(types_before[0]) != 5 and int(ids_before[0]) == best + 1
            if mode == "adopted":
                got = pl.select_clear(live, 0.03, 251, prev=best, adopt=True)
                assert got["pick"] == pick
                t, i = pl.best()
                assert (int(t[0]), int(i[0])) == (5, pick + 1)            # the pick's type: Random
            else:
                t, i = pl.best()
                assert (int(t[0]), int(i[0])) == (int(types_before[0]), best + 1)
            pl.move_real(live, sc["dt"], 1, best if mode == "best" else pick)
            pos, vel, _ = pl.real_state()
            setpoints[mode] = np.concatenate([np.asarray(pos).reshape(-1), np.asarray(vel).reshape(-1)])
        finally:
            pl.close()
    print("set-point with agent_id = best   ", setpoints["best"].tolist())
    print("set-point with agent_id = pick   ", setpoints["pick"].tolist())
    print("set-point with the pick adopted  ", setpoints["adopted"].tolist())
    _same_bits(setpoints["pick"], setpoints["best"], "agent_id selects gains only")
    assert (setpoints["adopted"].view(np.uint64) != setpoints["pick"].view(np.uint64)).any()


def test_pair_tick_adopt(pmaf, scenes, hip_lib):
    """shard.DualArmCoupling.pair_tick: adopt=False is what it was (bit-identical to a run that never heard of the
    argument); adopt=True reports the pair through get_best"""
    arms = scenes.dual_arm_scenes(n_agents=8, horizon=40, n_field=4)
    starts = np.stack([s["start"] for s in arms])
    sc = arms[0]
    runs = {}
    for mode in ("plain", "false", "true"):
        pl = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        try:
            cpl = pmaf.shard.DualArmCoupling(np.stack([s["obstacles"] for s in arms]), 0.1)
            pl.set_initial_position(starts)
            pl.start()
            rec = []
            for t in range(4):
                kw = {} if mode == "plain" else {"adopt": mode == "true"}
                out = cpl.pair_tick(pl, sc["dt"], sc["cost_gains"], sc["ws_limits"], margin=0.02, agent_radius=sc["radius"], **kw)
                rec.append((out["pair"], out["positions"].copy(), np.asarray(pl.best()[1]).copy()))
                if mode == "true":
                    np.testing.assert_array_equal(pl.best()[1], np.asarray(out["pair"]) + 1)
            runs[mode] = rec
        finally:
            pl.close()
    for (pa, xa, ba), (pb, xb, bb) in zip(runs["plain"], runs["false"]):
        assert pa == pb
        _same_bits(xb, xa, "pair_tick(adopt=False) set-points")
        np.testing.assert_array_equal(ba, bb)


def test_facade_audited_tick_equals_the_c_abi_sequence(pmaf, scenes, tmp_path, hip_lib):
    """tests/cpp/facade_audited_tick.cpp runs CfManager::planTickAudited over 5 ticks; the picks (and every other figure
    it prints) equal the six calls made through the binding"""
    N, cap, ticks, margin, horizon = 12, 101, 5, 0.05, 60
    sc = scenes.static1_scene(N, cap - 1)
    rvf = tmp_path / "rv.bin"
    np.ascontiguousarray(sc["random_vecs"]).tofile(rvf)
    exe = conftest.exe(os.path.join(ROOT, "tests", "cpp", "facade_audited_tick"))
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    out = subprocess.run([exe, str(N), str(cap), str(ticks), str(rvf), repr(margin), str(horizon)], capture_output=True,
                         check=True, env=conftest.binary_env(pmaf)).stdout.decode()
    lines = out.strip().split("\n")
    assert len(lines) == ticks
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        prev = None
        for t in range(ticks):
            f = lines[t].split()
            r = pl.audited_tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"], margin, horizon, prev=prev)
            prev = r["pick"]
            print(lines[t], "|", r)
            assert [int(v) for v in f[:5]] == [t, r["pick"], r["rule"], r["n_clear"], r["first_violation"]]
            _same_bits(np.array(f[5:7], dtype=float), [r["cost"], r["clearance"]], "cost, clearance")
            _same_bits(np.array(f[7:10], dtype=float), pl.last_next_pos, "set-point")
            assert int(f[10]) == pl.best_type()
        pl.stop()
    finally:
        pl.close()
