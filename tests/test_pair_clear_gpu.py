"""The joint selection on the GPU (pmaf_select_pair_clear / pmaf_select_clear_tracks, include/pmaf.h) through the C-ABI
against tests/pair_clear_reference.py at TOLERANCE 0: integers equal, doubles bit-equal, a NaN matched by a NaN. The
reference is fed the handle's own paths(), costs() and the live list, and takes its dot association from
pmaf_eval_order(), so the file passes unchanged under PMAF_VARIANT=rassoc. Scenes and parametrisation are
tests/pair_clear_cases.py's, the ones tests/test_pair_clear.py holds to every rule on the oracle's rollouts; every call
comes after one pmaf_evaluate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conftest
import pair_clear_cases as pc
import pair_clear_reference as ref
from test_cross_audit_gpu import rest_pair
from test_select_clear_gpu import _same_bits, _same_state, _state

pytestmark = pytest.mark.gpu

INT_KEYS = ("pair", "rule", "n_feasible", "n_clear", "first_violation", "steps")
DBL_KEYS = ("cost", "clearance", "obstacle_clearance", "worst_excess")
INF = float("inf")


def _evaluate(pl, sc):
    return pl.evaluate(sc["cost_gains"], sc["ws_limits"])


def _tables(pl):
    paths, n = pl.paths()
    paths = np.asarray(paths).reshape(pl.P, pl.N, pl.cap, 3)
    n = np.asarray(n).reshape(pl.P, pl.N)
    costs = np.asarray(pl.costs()).reshape(pl.P, pl.N)
    return paths.tolist(), n.tolist(), costs.tolist()


def _compare(got, want, tag):
    print(tag, "got", got)
    for k in INT_KEYS:
        assert got[k] == want[k], "%s: %s %r != %r" % (tag, k, got[k], want[k])
    for k in DBL_KEYS:
        _same_bits(got[k], want[k], k + " " + tag)


def _planner(pmaf, scenes, shape):
    P, N, M, H, ragged, _ = shape
    scs = pc.build_scenes(scenes, P, N, M, H, ragged)
    starts = np.stack([s["start"] for s in scs])
    pl = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    pl.set_initial_position(starts)
    pl.rollout()
    _evaluate(pl, scs[0])
    return pl, scs, pc.live_list(scenes, np.stack([s["obstacles"] for s in scs]))


class Shared:
    """the reference's audits and matrices of one handle state, computed once per key and never modified"""

    def __init__(self, pl, sc, live, order):
        self.pl, self.dt, self.live, self.order = pl, sc["dt"], np.asarray(live).tolist(), order
        self.rad = sc.get("radius", pc.RADIUS)
        self.paths, self.n, self.costs = _tables(pl)
        self.aud, self.mat = {}, {}

    def want(self, a, b, c, sep=pc.SEP):
        ka = (c["obstacle_margin"], c["horizon"], c["skip_trailing"])
        km = (a, b, c["horizon"], c["late"], sep)
        if ka not in self.aud:
            self.aud[ka] = ref.obstacle_side(self.paths, self.n, self.live, self.dt, self.rad, c["obstacle_margin"],
                                             c["horizon"], c["skip_trailing"], self.order)
        if km not in self.mat:
            self.mat[km] = ref.pair_side(self.paths[a], self.n[a], self.paths[b], self.n[b], c["horizon"], sep, c["late"],
                                         self.order)
        return ref.select_pair_clear(self.paths, self.n, self.live, self.costs, self.dt, self.rad, a, b, c["obstacle_margin"],
                                     c["horizon"], c["skip_trailing"], sep, c["pair_margin"], c["late"], c["prev_pair"],
                                     self.order, self.aud[ka], self.mat[km])

    def check(self, a, b, c, sep=pc.SEP, tag=""):
        got = self.pl.select_pair_clear(a, b, self.live, c["obstacle_margin"], c["horizon"], sep, c["pair_margin"],
                                        skip_trailing=c["skip_trailing"], late=c["late"], prev_pair=c["prev_pair"])
        _compare(got, self.want(a, b, c, sep), "%s %r" % (tag, c))
        return got


def _call(horizon, om, pm, skip=0, late=None, prev=None):
    return dict(horizon=horizon, obstacle_margin=om, pair_margin=pm, skip_trailing=skip, late=late, prev_pair=prev)


_SEEN = {}


def _run_shape(pmaf, scenes, hip_lib, shape):
    """every call of pc.calls(shape); returns the (rule, n_feasible regime) pairs seen. Run once per shape and session."""
    if shape in _SEEN:
        return _SEEN[shape]
    pl, scs, live = _planner(pmaf, scenes, shape)
    seen = set()
    try:
        N, (a, b) = shape[1], shape[5]
        sh = Shared(pl, scs[0], live, hip_lib.pmaf_eval_order())
        if shape[4]:
            assert len(set(sh.n[a])) > 1 and len(set(sh.n[b])) > 1, "the ragged case is meant to have paths of different lengths"
        for c in pc.calls(shape):
            got = sh.check(a, b, c, tag=pc.shape_id(shape))
            seen.add((got["rule"], 0 if got["n_feasible"] == 0 else (2 if got["n_feasible"] == N * N else 1)))
    finally:
        pl.close()
    _SEEN[shape] = seen
    return seen


@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.shape_id)
def test_shapes_horizons_margins_slacks(pmaf, scenes, hip_lib, shape):
    seen = _run_shape(pmaf, scenes, hip_lib, shape)
    print("(rule, n_feasible regime) seen:", sorted(seen))
    assert seen


def test_every_rule_and_every_n_feasible_regime_occurred(pmaf, scenes, hip_lib):
    seen = set()
    for shape in pc.SHAPES:
        seen |= _run_shape(pmaf, scenes, hip_lib, shape)
    print("(rule, n_feasible regime) over the whole parametrisation:", sorted(seen))
    assert {r for r, _ in seen} == {0, 1, 2}
    assert {g for _, g in seen} == {0, 1, 2}     # no pair feasible, some, all


def test_every_previous_pair_in_turn(pmaf, scenes, hip_lib):
    shape = pc.SHAPES[0]
    pl, scs, live = _planner(pmaf, scenes, shape)
    try:
        sh = Shared(pl, scs[0], live, hip_lib.pmaf_eval_order())
        for om, pm in ((-0.5, -0.5), (0.01, 0.0449), (3.0, -0.5)):
            for skip in (0, 1):
                none = sh.check(0, 1, _call(9, om, pm, skip))
                for prev in ((-1, -1), (-1, 2), (3, -1)):
                    assert sh.check(0, 1, _call(9, om, pm, skip, prev=prev)) == none or np.isnan(none["cost"])
                for i in range(5):
                    for j in range(5):
                        sh.check(0, 1, _call(9, om, pm, skip, prev=(i, j)))
    finally:
        pl.close()


def _rest_lists():
    # one moving sphere per list, test_hand_derived_moving_obstacle's, placed for an agent at the origin and for one at
    # (1, 0, 0): c(k) = 0.625 - 0.0625 k for both
    return np.array([[[1.0, 0.0, 0.0, -0.5, 0.0, 0.0, 0.25]], [[2.0, 0.0, 0.0, -0.5, 0.0, 0.0, 0.25]]])


def test_hand_derived(pmaf, scenes, hip_lib):
    """P = 2, N = 1, both agents at rest at (0, 0, 0) and (1, 0, 0): 7 identical points each, d = 1, separation 0.25 --
    the pair clearance is 0.75 at step 0; c(k) = 0.625 - 0.0625 k against each list's moving sphere. Literal
    expectations on both sides of each threshold."""
    pl, scs = rest_pair(pmaf, scenes, [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], 1)
    try:
        _evaluate(pl, scs[0])
        lists = _rest_lists()
        cost = np.asarray(pl.costs()).reshape(-1)
        assert np.isfinite(cost).all()

        def call(om, horizon, pm, skip=False):
            r = pl.select_pair_clear(0, 1, lists, om, horizon, 0.25, pm, skip_trailing=skip)
            print(om, horizon, pm, skip, r)
            return r["pair"], r["rule"], r["n_feasible"], r["n_clear"], r["clearance"], r["worst_excess"], r["first_violation"]

        # window 3: c = 0.5 on both sides, clear of 0.45; the pair keeps exactly 0.75
        assert call(0.45, 3, 0.75) == ((0, 0), 1, 1, (1, 1), 0.75, 0.0, (3, 3))
        assert call(0.45, 3, 0.5) == ((0, 0), 1, 1, (1, 1), 0.75, 0.5 - 0.45, (3, 3))
        assert call(0.45, 3, 0.8125) == ((0, 0), 2, 0, (1, 1), 0.75, -0.0625, (3, 3))
        # window 4 sees c = 0.4375 at step 3: blocked at margin 0.45, clear at margin 0.4375 (not below it)
        assert call(0.45, 4, 0.5) == ((0, 0), 2, 0, (0, 0), 0.75, 0.4375 - 0.45, (3, 3))
        assert call(0.4375, 4, 0.5) == ((0, 0), 1, 1, (1, 1), 0.75, 0.0, (4, 4))
        # the whole path: c = 0.25 at step 6
        assert call(0.25, 1000, 0.5) == ((0, 0), 1, 1, (1, 1), 0.75, 0.0, (7, 7))
        assert call(0.3125, 1000, 0.5) == ((0, 0), 2, 0, (0, 0), 0.75, 0.25 - 0.3125, (6, 6))
        # the lists' only obstacle skipped: nothing to audit, c = +inf, every agent clear at any margin
        r = pl.select_pair_clear(0, 1, lists, 5.0, 1000, 0.25, 0.5, skip_trailing=True)
        assert (r["rule"], r["n_clear"], r["obstacle_clearance"], r["worst_excess"], r["first_violation"]) == (
            1, (1, 1), (INF, INF), 0.25, (7, 7))
        _same_bits([r["cost"]], [cost[0] + cost[1]], "the pair's cost")
        assert r["steps"] == (0, 0)
    finally:
        pl.close()


def _twin_planner(pmaf, scenes, make):
    scs = [make(p) for p in range(2)]
    starts = np.stack([s["start"] for s in scs])
    pl = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    pl.set_initial_position(starts)
    pl.rollout()
    _evaluate(pl, scs[0])
    return pl, scs


def test_ties_go_to_the_row_major_first_pair(pmaf, scenes, hip_lib):
    """identical agents (same type, same gains) have identical paths and costs inside each population: every S ties and
    every g ties"""
    def make(p):
        sc = scenes.synthetic_scene(4, 20, 3, config_id=7, scene_id=0, dynamic=True, agent_types=[1, 1, 1, 1])
        sc["start"] = sc["start"] + np.array([0.0, 0.3 * p, 0.0])
        return sc
    pl, scs = _twin_planner(pmaf, scenes, make)
    try:
        costs = np.asarray(pl.costs()).reshape(2, 4)
        assert np.isfinite(costs).all() and (costs == costs[:, :1]).all(), costs
        live = np.stack([scenes.advance_live_obstacles(s["obstacles"]) for s in scs])
        sh = Shared(pl, scs[0], live, hip_lib.pmaf_eval_order())
        got = sh.check(0, 1, _call(21, -0.5, -0.5))
        assert (got["pair"], got["rule"], got["n_feasible"]) == ((0, 0), 1, 16)
        got = sh.check(0, 1, _call(21, -0.5, -0.5, prev=(2, 3)))      # S(m) >= 0.9 * S(prev): prev is kept
        assert (got["pair"], got["rule"]) == ((2, 3), 0)
        got = sh.check(0, 1, _call(21, 3.0, -0.5))                    # nobody clear: the g tie goes to (0, 0)
        assert (got["pair"], got["rule"], got["n_feasible"]) == ((0, 0), 2, 0)
        got = sh.check(0, 1, _call(21, -0.5, 3.0, prev=(1, 1)))
        assert (got["pair"], got["rule"], got["n_feasible"]) == ((0, 0), 2, 0)
    finally:
        pl.close()


def test_nan_paths_never_become_the_pick(pmaf, scenes, hip_lib):
    """test_select_clear_gpu's Had scene in both populations: agents 0 and 2 have NaN paths and costs, agent 1 is finite.
    While a comparable pair exists the pair is (1, 1); a NaN clearance is never feasible and takes no part in rule 2."""
    def make(p):
        sc = scenes.synthetic_scene(3, 60, 1, 9, 2)
        sc["start"] = np.array([-0.44, 0.3 * p, 0.7])
        sc["goal"] = np.array([0.6, 0.3 * p, 0.7])
        sc["obstacles"][0] = [0.0, 0.3 * p, 0.7, 0, 0, 0, 0.05]
        sc["agent_types"] = np.array([6, 1, 6], dtype=np.int32)
        return sc
    pl, scs = _twin_planner(pmaf, scenes, make)
    try:
        paths, n = pl.paths()
        paths, n = np.asarray(paths).reshape(2, 3, pl.cap, 3), np.asarray(n).reshape(2, 3)
        nan_agent = [[bool(np.isnan(paths[p, a, :n[p, a]]).any()) for a in range(3)] for p in range(2)]
        print("NaN path per agent", nan_agent, "costs", np.asarray(pl.costs()).tolist())
        assert nan_agent == [[True, False, True]] * 2
        live = np.stack([s["obstacles"] for s in scs])
        sh = Shared(pl, scs[0], live, hip_lib.pmaf_eval_order())
        for om, pm in ((-0.5, -0.5), (0.01, 0.05)):
            for horizon in (5, 30, 61):
                for prev in (None, (0, 0), (1, 1), (2, 1)):
                    got = sh.check(0, 1, _call(horizon, om, pm, prev=prev))
                    assert got["pair"] == (1, 1) and got["rule"] in (0, 1), (om, pm, horizon, prev)
        got = sh.check(0, 1, _call(61, -0.5, 10.0))          # nothing feasible: rule 2 among the non-NaN clearances only
        assert got["rule"] == 2 and not np.isnan(got["clearance"])
    finally:
        pl.close()


def test_equals_select_pair_where_every_agent_is_clear(pmaf, scenes, hip_lib):
    """a far list, horizon >= cap, no previous pair: where select_pair reports a feasible pair the joint call returns
    its results bit for bit, step against step and slacked; n_feasible never grows with a margin or a slack"""
    shape = pc.SHAPES[1]
    pl, scs, live = _planner(pmaf, scenes, shape)
    try:
        far = np.array(live, copy=True)
        far[:, :, 0:3] = 9.0
        far[:, :, 3:6] = 0.0
        seen = 0
        for late in (None, (0, 0), (2, 1)):
            last = None
            for pm in (-0.5, -0.1485, -0.1477, -0.1472, 3.0):
                sp = pl.select_pair(0, 1, pc.SEP, pm) if late is None else pl.select_pair_slack(0, 1, pc.SEP, pm, late[0], late[1])
                got = pl.select_pair_clear(0, 1, far, 0.05, pl.cap + 3, pc.SEP, pm, late=late)
                print(late, pm, sp, got)
                assert got["n_clear"] == (pl.N, pl.N)
                if sp["feasible"]:
                    seen += 1
                    assert got["pair"] == sp["pair"] and got["rule"] == 1
                    _same_bits([got["cost"], got["clearance"]], [sp["cost"], sp["clearance"]], "select_pair's results")
                    if late is not None:
                        assert got["steps"] == sp["steps"]
                assert last is None or got["n_feasible"] <= last
                last = got["n_feasible"]
        assert seen >= 6
        for key, values in (("om", (-0.5, 0.1, 0.10827, 0.11, 3.0)), ("late", ((0, 0), (1, 0), (1, 3), (9, 9)))):
            last = None
            for v in values:
                if key == "om":
                    got = pl.select_pair_clear(0, 1, live, v, pl.cap, pc.SEP, -0.1477, skip_trailing=True)
                else:
                    got = pl.select_pair_clear(0, 1, live, 0.10827, pl.cap, pc.SEP, -0.1477, skip_trailing=True, late=v)
                assert last is None or got["n_feasible"] <= last, (key, v)
                last = got["n_feasible"]
    finally:
        pl.close()


def _dual_arm(pmaf, scenes):
    arms = scenes.dual_arm_scenes(n_agents=8, horizon=40, n_field=4)
    for s in arms:   # different gains per agent: move_real's agent_id matters too
        s["k_attr"] = np.linspace(2.0, 6.0, 8)
        s["k_damp"] = np.linspace(2.5, 4.0, 8)
    return arms, np.stack([s["start"] for s in arms])


def test_calls_without_adoption_between_ticks_change_nothing(pmaf, scenes, hip_lib):
    arms, starts = _dual_arm(pmaf, scenes)
    sc = arms[0]
    lists = [np.stack([s["obstacles"] for s in arms])]
    for t in range(6):
        nxt = np.stack([scenes.advance_live_obstacles(o) for o in lists[-1]])
        nxt[:, :-1, 3:6] = 0.02 * (t + 1)
        lists.append(nxt)
    tracks = np.zeros((2, 41, 3))
    tracks[:, :, 2] = 0.7
    runs = []
    for select in (False, True):
        pl = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        try:
            pl.set_initial_position(starts)
            rec = []
            for t in range(6):
                b = pl.tick(lists[t], sc["dt"], sc["cost_gains"], sc["ws_limits"])
                rec.append((np.asarray(b).copy(), pl.last_next_pos.copy(), pl.last_next_vel.copy()))
                if select:   # given the list of the FOLLOWING tick: it must not become the resident one
                    r = pl.select_pair_clear(0, 1, lists[t + 1], 0.02, 30 if t % 2 else 1000, 0.15, 0.02, skip_trailing=t % 3 == 0,
                                             late=(1, 2) if t % 2 else None, prev_pair=None if t == 0 else tuple(int(v) for v in b))
                    assert 0 <= r["pair"][0] < pl.N
                    r = pl.select_clear_tracks(1, lists[t + 1], 0.02, 30, tracks, [41, 7], 0.15, 0.02, track_cost=[1.0, 2.0])
                    assert 0 <= r["pair"][1] < 2
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
    """two handles, 6 ticks of the intended sequence: A adopts inside the call, B calls with adopt = 0 and then
    pmaf_adopt_best(pair). Results, state and set-points are bit-identical; a third population would be left alone
    (-1 entries), here both populations adopt."""
    arms, starts = _dual_arm(pmaf, scenes)
    sc = arms[0]
    obs = np.stack([s["obstacles"] for s in arms])
    A = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
    B = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
    try:
        for pl in (A, B):
            pl.set_initial_position(starts)
            pl.start()
        prev = None
        for t in range(6):
            live = np.stack([scenes.advance_live_obstacles(o) for o in obs])
            om = (0.02, 0.06, 0.1)[t % 3]
            out = []
            for pl in (A, B):
                pl.stop()
                _evaluate(pl, sc)
                r = pl.select_pair_clear(0, 1, live, om, 30, 0.15, 0.02, skip_trailing=True, late=(1, 1) if t % 2 else None,
                                         prev_pair=prev, adopt=pl is A)
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


def test_calls_of_every_kind_alternate_on_one_handle(pmaf, scenes, hip_lib):
    """the cross audit's scratch and the select scratch are shared and grow-only: calls of every kind in rotation,
    small and large matrices alternating, each compared with its first answer"""
    shape = pc.SHAPES[3]
    pl, scs, live = _planner(pmaf, scenes, shape)
    try:
        rng = np.random.default_rng(11)
        tracks = rng.uniform(-1.0, 1.0, (40, pl.cap, 3))
        ntp = np.full(40, pl.cap, dtype=np.int32)
        kinds = [
            lambda: pl.select_pair_clear(0, 1, live, 0.01, 9, pc.SEP, 0.0449, skip_trailing=True),
            lambda: pl.cross_audit(0, 1, pc.SEP, step=True),
            lambda: pl.select_clear_tracks(0, live, 0.01, 9, tracks[:1], ntp[:1], pc.SEP, -0.5),
            lambda: pl.select_clear(live, 0.01, 9),
            lambda: pl.select_pair_clear(1, 0, live, 0.01, 4, pc.SEP, 0.0449, late=(1, 2), prev_pair=(3, 4)),
            lambda: pl.cross_audit_slack(0, 1, pc.SEP, 2, 1, steps=True),
            lambda: pl.select_clear_tracks(1, live, -0.5, 9, tracks, ntp, pc.SEP, -0.5, track_cost=np.arange(40.0), late=(0, 1)),
            lambda: pl.select_pair(0, 1, pc.SEP, 0.0449),
            lambda: pl.cross_audit_tracks(0, tracks, ntp, pc.SEP, step=True),
            lambda: pl.select_pair_slack(0, 1, pc.SEP, 0.0449, 1, 1),
        ]

        def flat(r):
            vals = r.values() if isinstance(r, dict) else (r if isinstance(r, tuple) else (r,))
            return np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in vals])

        first = [flat(k()) for k in kinds]
        for rnd in range(2):
            order = list(range(len(kinds)))[::-1] if rnd else list(range(len(kinds)))
            for i in order:
                _same_bits(flat(kinds[i]()), first[i], "kind %d round %d" % (i, rnd))
    finally:
        pl.close()


@pytest.mark.parametrize("N,n_tracks", [(5, 1), (5, 33), (33, 33)])
def test_tracks_variant(pmaf, scenes, hip_lib, N, n_tracks):
    shape = (2, N, 2, 24, False, (0, 1))
    P, _, M, H, ragged, _ = shape
    scs = pc.build_scenes(scenes, P, N, M, H, ragged)
    starts = np.stack([s["start"] for s in scs])
    pl = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    try:
        pl.set_initial_position(starts)
        pl.rollout()
        _evaluate(pl, scs[0])
        live = pc.live_list(scenes, np.stack([s["obstacles"] for s in scs]))
        paths, n, costs = _tables(pl)
        cap = pl.cap
        rng = np.random.default_rng(5)
        # tracks around population 1's start: a random walk of 2 cm steps, 0, 1, a middle number and cap points
        tracks = np.asarray(scs[1]["start"]) + np.cumsum(rng.uniform(-0.02, 0.02, (n_tracks, cap, 3)), axis=1)
        ntp = np.asarray(([cap, 0, 1, cap // 2] * n_tracks)[:n_tracks], dtype=np.int32)
        for t in range(n_tracks):
            tracks[t, ntp[t]:] = np.nan           # rows past the count are not read: a NaN there would be refused
        tcost = rng.choice([1.0, 2.0, 2.0, 0.5], n_tracks)
        order = hip_lib.pmaf_eval_order()
        rules = set()
        k = 0
        for horizon in (1, 3, H // 2, H + 6):
            for om, pm in ((-0.5, -0.5), (0.01, 0.03), (0.01, 0.06), (3.0, 0.03), (-0.5, 3.0)):
                for late in (None, (1, 2)):
                    for tc in (None, tcost):
                        prev = None if k % 2 == 0 else ((3 * k) % N, k % n_tracks)
                        k += 1
                        got = pl.select_clear_tracks(0, live, om, horizon, tracks, ntp, pc.SEP, pm, track_cost=tc,
                                                     skip_trailing=k % 3 == 0, late=late, prev_pair=prev)
                        want = ref.select_clear_tracks(paths, n, live.tolist(), costs, scs[0]["dt"], pc.RADIUS, 0, om, horizon,
                                                       k % 3 == 0, tracks.tolist(), ntp.tolist(), None if tc is None else tc.tolist(),
                                                       pc.SEP, pm, late, prev, order)
                        _compare(got, want, "tracks horizon %d om %r pm %r late %r prev %r" % (horizon, om, pm, late, prev))
                        assert got["n_clear"][1] == n_tracks
                        rules.add(got["rule"])
        print("rules seen", sorted(rules))
        assert {1, 2} <= rules
    finally:
        pl.close()


def test_pair_tick_clear_equals_the_explicit_sequence(pmaf, scenes, hip_lib):
    """shard.DualArmCoupling.pair_tick(clear=...) over 4 ticks against the calls it stands for; without `clear` it is
    the five-call sequence it was"""
    arms, starts = _dual_arm(pmaf, scenes)
    sc = arms[0]
    obs0 = np.stack([s["obstacles"] for s in arms])
    for mode in ("clear", "clear_late", "plain"):
        A = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        B = pmaf.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        try:
            ca = pmaf.shard.DualArmCoupling(obs0, 0.1)
            cb = pmaf.shard.DualArmCoupling(obs0, 0.1)
            for pl in (A, B):
                pl.set_initial_position(starts)
                pl.start()
            late = (1, 2) if mode == "clear_late" else None
            prev = None
            for t in range(4):
                kw = {} if mode == "plain" else {"clear": dict(margin=0.03, horizon=30), "late": late, "adopt": True}
                out = ca.pair_tick(A, sc["dt"], sc["cost_gains"], sc["ws_limits"], margin=0.02, agent_radius=sc["radius"], **kw)
                B.stop()
                best = _evaluate(B, sc)
                if mode == "plain":
                    r = B.select_pair(0, 1, sc["radius"] + 0.1, 0.02)
                    obs = cb.coupled_obstacles(B.real_state()[0])
                else:
                    obs = cb.coupled_obstacles(B.real_state()[0])
                    r = B.select_pair_clear(0, 1, obs, 0.03, 30, sc["radius"] + 0.1, 0.02, skip_trailing=True, late=late,
                                            prev_pair=prev, adopt=True)
                    prev = r["pair"]
                    assert out["rule"] == r["rule"] and out["n_feasible"] == r["n_feasible"]
                    _same_bits([out["worst_excess"]], [r["worst_excess"]], "worst excess")
                pair = r["pair"] if r["pair"][0] >= 0 else tuple(int(b) for b in best)
                B.move_real(obs, sc["dt"], 1, np.asarray(pair, dtype=np.int32))
                pos, vel, _ = B.real_state()
                B.reset_agents(pos, vel, obs)
                B.start()
                print(mode, "tick", t, out["pair"], pair)
                assert out["pair"] == tuple(pair)
                _same_bits([out["cost"], out["clearance"]], [r["cost"], r["clearance"]], "pair cost and clearance")
                _same_bits(out["positions"], pos, "set-points")
                _same_state(_state(A), _state(B), "%s tick %d" % (mode, t))
        finally:
            A.close()
            B.close()


@pytest.mark.parametrize("late", [None, (2, 1)])
def test_facade_select_clear_against_equals_the_c_abi_sequence(pmaf, scenes, tmp_path, hip_lib, late):
    """tests/cpp/facade_joint_tick.cpp runs CfManager::selectClearAgainst inside the intended tick over 5 ticks; every
    figure it prints equals the same calls made through the binding (pmaf_select_clear_tracks with skip_trailing and
    the previous tick's pair)"""
    N, cap, ticks, margin, horizon, sep, pm = 12, 101, 5, 0.05, 60, 0.15, 0.04
    sc = scenes.static1_scene(N, cap - 1)
    rvf = tmp_path / "rv.bin"
    np.ascontiguousarray(sc["random_vecs"]).tofile(rvf)
    exe = conftest.exe(os.path.join(conftest.ROOT, "tests", "cpp", "facade_joint_tick"))
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    lt = (-1, -1) if late is None else late
    out = subprocess.run([exe, str(N), str(cap), str(ticks), str(rvf), repr(margin), str(horizon), repr(sep), repr(pm),
                          str(lt[0]), str(lt[1])], capture_output=True, check=True, env=conftest.binary_env(pmaf)).stdout.decode()
    lines = out.strip().split("\n")
    assert len(lines) == ticks
    k = np.arange(cap, dtype=np.float64)
    tracks = np.zeros((2, cap, 3))
    tracks[0] = np.stack([-0.6 + 0.002 * k, 0.25 - 0.001 * k, np.full(cap, 0.75)], axis=1)
    tracks[1, :5] = np.stack([-0.6 + 0.002 * k[:5], np.full(5, -0.3), np.full(5, 0.75)], axis=1)
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        prev = (-1, -1)
        for t in range(ticks):
            f = lines[t].split()
            pl.stop()
            pl.evaluate(sc["cost_gains"], sc["ws_limits"])
            r = pl.select_clear_tracks(0, sc["obstacles"], margin, horizon, tracks, [cap, 5], sep, pm, skip_trailing=True,
                                       late=late, prev_pair=prev, adopt=True)
            pl.move_real(sc["obstacles"], sc["dt"], 1, r["pair"][0])
            pos, vel, _ = pl.real_state()
            pl.reset_agents(pos, vel, sc["obstacles"])
            pl.start()
            prev = r["pair"]
            print(lines[t], "|", r)
            assert [int(v) for v in f[:9]] == [t, r["pair"][0], r["pair"][1], r["rule"], r["n_feasible"], r["n_clear"][0],
                                               r["first_violation"][0], r["steps"][0], r["steps"][1]]
            _same_bits(np.array(f[9:13], dtype=float), [r["cost"], r["clearance"], r["obstacle_clearance"][0], r["worst_excess"]],
                       "cost, clearance, obstacle clearance, worst excess")
            _same_bits(np.array(f[13:16], dtype=float), pos, "set-point")
            assert int(f[16]) == pl.best_type()
        pl.stop()
    finally:
        pl.close()


def test_argument_validation(pmaf, scenes, hip_lib):
    shape = pc.SHAPES[0]
    pl, scs, live = _planner(pmaf, scenes, shape)
    try:
        L, h = hip_lib, pl._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        obs = np.ascontiguousarray(live, dtype=np.float64)
        tracks = np.zeros((2, pl.cap, 3))
        ntp = np.array([pl.cap, 3], dtype=np.int32)
        oi = {k: np.full(2, -7, dtype=np.int32) for k in ("pair", "rule", "n_feasible", "n_clear", "fv", "steps")}
        od = {k: np.full(2, -7.0) for k in ("cost", "clearance", "oc", "we")}

        def outs(drop=()):
            order = ["pair", "rule", "n_feasible", "n_clear", "cost", "clearance", "oc", "fv", "we", "steps"]
            return [None if k in drop else (oi[k].ctypes.data_as(ip) if k in oi else od[k].ctypes.data_as(dp)) for k in order]

        def pair_call(h_=h, a=0, b=1, o=obs, om=0.05, horizon=5, sep=0.15, pm=0.02, late=None, prev=None, drop=()):
            lt = None if late is None else np.asarray(late, dtype=np.int32).ctypes.data_as(ip)
            pv = None if prev is None else np.asarray(prev, dtype=np.int32).ctypes.data_as(ip)
            return L.pmaf_select_pair_clear(h_, a, b, None if o is None else o.ctypes.data_as(dp), om, horizon, 0, sep, pm, lt, pv, 0,
                                            *outs(drop))

        def track_call(pop=0, n_tracks=2, n=ntp, tc=None, prev=None, horizon=5):
            pv = None if prev is None else np.asarray(prev, dtype=np.int32).ctypes.data_as(ip)
            return L.pmaf_select_clear_tracks(h, pop, obs.ctypes.data_as(dp), 0.05, horizon, 0, n_tracks, tracks.ctypes.data_as(dp),
                                              n.ctypes.data_as(ip), None if tc is None else tc.ctypes.data_as(dp), 0.15, 0.02, None,
                                              pv, 0, *outs())

        assert pair_call(h_=None) == -1 and pair_call(o=None) == -1 and pair_call(drop=("pair",)) == -1
        for a, b in ((0, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (0, -1)):
            assert pair_call(a=a, b=b) == -1, (a, b)
        for horizon in (0, -1, -2 ** 31):
            assert pair_call(horizon=horizon) == -1 and track_call(horizon=horizon) == -1, horizon
        for late in ((-1, 0), (0, -1)):
            assert pair_call(late=late) == -1, late
        for prev in ((5, 0), (0, 5), (-2, 0), (0, -2)):
            assert pair_call(prev=prev) == -1, prev
        for prev in ((5, 0), (0, 2), (-2, 0), (0, -2)):
            assert track_call(prev=prev) == -1, prev
        for kw in (dict(om=float("nan")), dict(pm=float("inf")), dict(sep=float("nan"))):
            assert pair_call(**kw) == -1, kw
        bad = obs.copy()
        bad[1, 1, 4] = np.nan
        assert pair_call(o=bad) == -1 and b"range" in L.pmaf_last_error()
        assert track_call(pop=2) == -1 and track_call(n_tracks=0) == -1
        assert track_call(n=np.array([pl.cap + 1, 3], dtype=np.int32)) == -1
        assert track_call(tc=np.array([1.0, np.nan])) == -1
        assert all((v == -7).all() for v in oi.values()) and all((v == -7.0).all() for v in od.values())   # nothing written
        # every optional output NULL in turn: the others unchanged
        assert pair_call() == 0 and track_call() == 0 and track_call(prev=(4, 1), tc=np.array([1.0, 2.0])) == 0
        assert pair_call(prev=(4, 4), late=(0, 3)) == 0
        full = {k: v.copy() for k, v in list(oi.items()) + list(od.items())}
        for drop in ("rule", "n_feasible", "n_clear", "cost", "clearance", "oc", "fv", "we", "steps"):
            for v in oi.values():
                v[:] = -7
            for v in od.values():
                v[:] = -7.0
            assert pair_call(prev=(4, 4), late=(0, 3), drop=(drop,)) == 0
            for k, v in list(oi.items()) + list(od.items()):
                if k == drop:
                    assert (v == -7).all(), k
                else:
                    _same_bits(v.astype(np.float64), full[k].astype(np.float64), "optional output %s without %s" % (k, drop))
    finally:
        pl.close()


def test_refused_after_an_abandoned_tick(pmaf, scenes, hip_lib, monkeypatch):
    """test_select_clear_gpu's fault injection: a tick that ran into its time limit leaves the handle abandoned until
    pmaf_stop, and both calls refuse it"""
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
        tracks = np.zeros((1, pl.cap, 3))
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_pair_clear(0, 1, obs, 0.05, 5, 0.15, 0.02)
        assert e.value.code == -3, str(e.value)
        with pytest.raises(pmaf.PmafError) as e:
            pl.select_clear_tracks(0, obs, 0.05, 5, tracks, [3], 0.15, 0.02)
        assert e.value.code == -3, str(e.value)
        pl.stop()
        r = pl.select_pair_clear(0, 1, obs, 0.05, 5, 0.15, 0.02, adopt=True)
        assert 0 <= r["pair"][0] < 512 and 0 <= r["pair"][1] < 512
        np.testing.assert_array_equal(pl.best()[1], np.asarray(r["pair"]) + 1)
    finally:
        pl.close()
