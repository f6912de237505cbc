"""The manager step's selection at every shape, on the CPU: the oracle (oracle/pmaf_oracle.c, through orc.OraclePlanner)
taken through the designed selections of tests/hp_select.py -- exact ties, the only minimum and the stored best agent
placed by agent index -- and held to the independent high-precision reference. The same cases run on the kernels in
tests/test_hp_select_gpu.py; here they are shown to be decidable by the reference alone (undecidable share 0), to take
both sides of the evaluation's branches, and to have teeth: planners that select by a plausible wrong rule fail, each
on a named case. Run with -s to see the per-case report.
"""
import numpy as np
import pytest

import hp_reference as hp
import hp_select as hs
import hp_shadow as sh
from test_hp_reference import PopOracles

_DONE = {}


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


def _oracle(orc):
    return lambda sc: orc.OraclePlanner(sc, mgr_init_pos=sc["start"])


def _case(orc, scenes, N, kind, where=None, entry="tick", make=None, seed=hs.SEED, **over):
    """one designed case on the oracle (or on make(scene)): (Stats, rollout Stats); the oracle's runs are kept for the
    coverage test. A planner from `make` is handed the layout designed from the ORACLE's probe, and the layout's own
    by-construction assertion is not raised for it: what the reference found is in the returned Stats"""
    key = (N, kind, where, entry, seed, tuple(sorted(over)))
    if make is None and key in _DONE:
        return _DONE[key]
    A = hp.Arith("xact")
    st, rs = sh.Stats(hs.case_id(N, kind, where, entry)), sh.Stats("rollouts")
    if make is not None and N > 1 and kind not in ("all_same", "zero"):
        hs.probed(_oracle(orc), scenes, N, seed, A, "oracle", **over)
    try:
        hs.designed_case(make or _oracle(orc), scenes, N, seed, kind, A, st, "oracle", where=where, entry=entry,
                         rollout_stats=rs, **over)
    except AssertionError:
        if make is None:
            raise
    if make is None:
        _DONE[key] = (st, rs)
    return st, rs


ALL = ([(N, k, None, "tick") for N, k in hs.TIE_CASES] + [(N, k, w, "tick") for N, k, w in hs.PRIOR_CASES] +
       [(N, k, w, "evaluate") for N, k, w in hs.EVALUATE_CASES])


@pytest.mark.parametrize("N,kind,where,entry", ALL, ids=[hs.case_id(*c) for c in ALL])
def test_designed_selection(orc, scenes, N, kind, where, entry):
    """the oracle selects the layout's index; every cost, the selection, best_type and the real step within the
    reference's bound, decided by the reference alone"""
    st, rs = _case(orc, scenes, N, kind, where, entry)
    hs.assert_decided(st, rs, N)


@pytest.mark.parametrize("N,kind,seed", hs.RECORD_CASES)
def test_winner_is_a_random_agent(orc, scenes, N, kind, seed):
    """the condition on these cases' inputs: the selected agent is a Random agent, agent 0 is not, and the real agent
    latches a rotation vector in the compared step"""
    st, rs = _case(orc, scenes, N, kind, seed=seed)
    hs.assert_decided(st, rs, N)
    sc = hs.selection_scene(scenes, N, seed)
    pr = hs.probed(_oracle(orc), scenes, N, seed, hp.Arith("xact"), "oracle")
    assert sc["agent_types"][pr.w] == hp.RANDOM and sc["agent_types"][0] != hp.RANDOM
    assert st.seen.get("known") == {False}, st.report()      # every obstacle inside the shell was latched in this step


def test_near_goal(orc, scenes):
    """agents on both sides of approach_dist: the goal-distance term of the cost is dropped for some of them"""
    st, rs = _case(orc, scenes, 65, "plain", **hs.near_goal(scenes))
    hs.assert_decided(st, rs, 65)
    assert st.seen.get("goal_cost") == {True, False}, st.report()


# ---------------------------------------------------------------------------------------------------------------------
# P populations
# ---------------------------------------------------------------------------------------------------------------------
class Pops(PopOracles):
    """tests/test_hp_reference.py's P oracle planners as one P-population planner, with the rest of the surface
    hp_select.run_selection drives. mix: applied to the list of per-population winners before they are returned and used
    for the real agents' steps; min_obs_of: the population whose min_obs_dist enters population p's costs (mutants)"""

    def __init__(self, orc, scs, mix=None, min_obs_of=None):
        PopOracles.__init__(self, orc, scs)
        self.scs, self.mix, self.min_obs_of, self._costs = scs, mix or (lambda b: b), min_obs_of, None

    def reset_agents(self, pos, vel, obs):
        for q, x, v, o in zip(self.pl, np.reshape(pos, (self.P, 3)), np.reshape(vel, (self.P, 3)), np.reshape(obs, (self.P, -1, 7))):
            q.reset_agents(x, v, o)

    def rollout(self):
        self._each("rollout")

    def tick(self, obs, dt, cost_gains, ws):
        obs = np.reshape(obs, (self.P, -1, 7))
        best = [q.evaluate(cost_gains, ws) for q in self.pl]
        self._costs = np.stack(self._each("costs"))
        if self.min_obs_of is not None:
            mo = np.stack(self._each("min_obs_dist"))
            self._costs = np.stack([self._costs[p] - cost_gains[2] / mo[p] + cost_gains[2] / mo[self.min_obs_of(p)]
                                    for p in range(self.P)])
            best = [int(np.argmin(c)) for c in self._costs]
        best = self.mix(best)
        for p, q in enumerate(self.pl):
            if best[p] + 1 != q.best_id():       # (a mutant's choice: stored as the oracle would store its own)
                q.set_best(best[p] + 1, sh.agent_types(self.scs[p])[best[p]], self.scs[p]["random_vecs"][best[p]])
            q.move_real(obs[p], dt, 1, best[p])
            pos, vel, _ = q.real_state()
            q.reset_agents(pos, vel, obs[p])
            q.rollout()
        return np.array(best)

    def costs(self):
        return self._costs if self._costs is not None else np.stack(self._each("costs"))


def _pops(orc, scenes, N, **mutation):
    A = hp.Arith("xact")
    st, rs = sh.Stats("P = 3, N = %d" % N), sh.Stats("rollouts")
    scs = hs.population_scenes(scenes, N)
    pl = Pops(orc, scs, **mutation)
    try:
        best = hs.run_populations(pl, scs, A, st, rollout_stats=rs)
    finally:
        pl.close()
    return st, rs, best


@pytest.mark.parametrize("N", [65, 321])
def test_three_populations(orc, scenes, N):
    """three populations with different fields, gains and goals: the reference's three winners are distinct indices, so
    a planner that mixes up the populations' offsets cannot pass"""
    st, rs, best = _pops(orc, scenes, N)
    hs.assert_decided(st, rs, N, 3)
    assert len(set(best)) == 3, best


# ---------------------------------------------------------------------------------------------------------------------
# branch coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_selection_branch_coverage(orc, scenes):
    """over the designed cases, both outcomes of the argmin scan, the hysteresis, the workspace test and the
    goal-distance test were decided"""
    seen = {}
    runs = [_case(orc, scenes, *c)[0] for c in ALL if c[0] <= 129]
    runs.append(_case(orc, scenes, 65, "plain", **hs.near_goal(scenes))[0])
    for st in runs:
        for k, v in st.seen.items():
            seen.setdefault(k, set()).update(v)
    for b in ("argmin", "hysteresis", "ws", "goal_cost"):
        assert seen.get(b) == {True, False}, (b, seen.get(b))


# ---------------------------------------------------------------------------------------------------------------------
# teeth: planners that select by a plausible wrong rule
# ---------------------------------------------------------------------------------------------------------------------
def _first_min(c):
    return int(np.argmin(c))


class Rule:
    """evaluateAgents' selection with replaceable parts: the argmin, the hysteresis test, the stored best agent's cost,
    and the agent whose type / random vectors go into the stored copy"""

    def __init__(self, argmin=_first_min, take=lambda cm, cb: cm < 0.9 * cb, prior_cost=lambda c, i: c[i - 1],
                 type_of=lambda i: i, rand_of=lambda i: i, min_obs_of=None, min_cost=lambda c, m: c[m]):
        self.argmin, self.take, self.prior_cost, self.type_of, self.rand_of = argmin, take, prior_cost, type_of, rand_of
        self.min_cost = min_cost
        self.min_obs_of = min_obs_of             # agent index -> the agent whose min_obs_dist enters its cost


class RuledOracle:
    """an oracle planner whose evaluate / tick select by `rule` (tick = evaluate, move the real agent, reset, roll out:
    oracle/pmaf_oracle.c orc_tick)"""

    def __init__(self, orc, scene, rule):
        self.inner = orc.OraclePlanner(scene, mgr_init_pos=scene["start"])
        self.sc, self.rule, self.rand, self._costs = scene, rule, None, None

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def set_best(self, ids, types, rand_vecs=None):
        self.rand = None if rand_vecs is None else np.array(rand_vecs, dtype=np.float64).reshape(-1, 3)
        self.inner.set_best(ids, types, self.rand)

    def evaluate(self, cost_gains, ws):
        prev, ptype = self.inner.best_id(), self.inner.best_type()
        self.inner.evaluate(cost_gains, ws)
        c, r = self.inner.costs(), self.rule
        if r.min_obs_of is not None:
            mo = self.inner.min_obs_dist()
            c = c - cost_gains[2] / mo + cost_gains[2] / mo[[r.min_obs_of(a) for a in range(len(c))]]
        self._costs = c
        m = r.argmin(c)
        if prev and not r.take(r.min_cost(c, m), r.prior_cost(c, prev)):
            self.inner.set_best(prev, ptype, self.rand)
            return prev - 1
        self.rand = self.sc["random_vecs"][r.rand_of(m)]
        self.inner.set_best(m + 1, sh.agent_types(self.sc)[r.type_of(m)], self.rand)
        return m

    def costs(self):
        return self._costs if self._costs is not None else self.inner.costs()

    def tick(self, obs, dt, cost_gains, ws):
        best = self.evaluate(cost_gains, ws)
        self.inner.move_real(obs, dt, 1, best)
        pos, vel, _ = self.inner.real_state()
        self.inner.reset_agents(pos, vel, obs)
        self.inner.rollout()
        return best


def _last_min(c):
    return len(c) - 1 - int(np.argmin(c[::-1]))


def _lane_major(c):
    return min(range(len(c)), key=lambda a: (c[a], a % 64, a))


def _down64(c):
    n = len(c) // 64 * 64
    return int(np.argmin(c[:n])) if n else int(np.argmin(c))


# mutant -> (rule, the designed cases that must catch it, what the failure names)
MUTANTS = {
    "last minimum among tied agents": (Rule(argmin=_last_min), [(129, "next_slot"), (577, "next_pass"), (64, "last"), (65, "all_same")], "best index"),
    "lane-major first minimum": (Rule(argmin=_lane_major), [(129, "lane_order"), (257, "lane_order")], "best index"),
    "minimum over the first 256 agents": (Rule(argmin=lambda c: int(np.argmin(c[:256]))), [(257, "tail"), (321, "tail"), (577, "tail")], "best index"),
    "minimum over N rounded down to 64": (Rule(argmin=_down64), [(65, "tail"), (129, "tail"), (255, "tail")], "best index"),
    "hysteresis with <=": (Rule(take=lambda cm, cb: cm <= 0.9 * cb), [(129, "zero", "mid")], "best index"),
    "hysteresis without the 0.9": (Rule(take=lambda cm, cb: cm < cb), [(321, "keep_near", "high"), (63, "keep_near", "last")], "best index"),
    "prior cost from (id - 1) % 64": (Rule(prior_cost=lambda c, i: c[(i - 1) % 64]), [(129, "keep_dup", "mid"), (129, "switch", "mid"), (321, "switch", "high")], "best index"),
    "winner's type from index 0": (Rule(type_of=lambda i: 0), [c + (None, "tick", None) for c in hs.RECORD_CASES], "best_type"),
    "winner's random vectors from index 0": (Rule(rand_of=lambda i: 0), [c + (None, "tick", None) for c in hs.RECORD_CASES], "real "),
    # (the min_obs stream of the cost assembly: slot 0's value for the later slots, the first pass's for the later ones)
    "min_obs_dist from a % 64": (Rule(min_obs_of=lambda a: a % 64), [(65, "tail"), (129, "next_slot"), (321, "tail")], "cost["),
    "min_obs_dist from a % 256": (Rule(min_obs_of=lambda a: a % 256), [(257, "tail"), (321, "plain"), (577, "next_pass")], "cost["),
    "hysteresis reads the argmin's cost from min_idx % 64": (Rule(min_cost=lambda c, m: c[m % 64]), [(129, "switch_far", "mid"), (321, "switch_far", "high")], "best index"),
}


def test_true_rule_passes_through_the_wrapper(orc, scenes):
    """the wrapper the mutants run in, with the true rule: passes (so a mutant's failure is its rule's)"""
    for c in [(129, "keep_dup", "mid"), (321, "tail"), (321, "switch", "high", "evaluate"), (129, "switch_far", "mid")]:
        st, rs = _case(orc, scenes, *c, make=lambda sc: RuledOracle(orc, sc, Rule()))
        hs.assert_decided(st, rs, c[0])


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_caught(orc, scenes, name):
    """on each named case the independent reference itself flags the mutant: a `best index`, `best_type`, `cost[` or
    real-step entry among the Stats' failures"""
    rule, cases, what = MUTANTS[name]
    for c in cases:
        kw = {}
        if len(c) == 6:                          # a RECORD_CASES entry: (N, layout, seed)
            c, kw = c[:2], dict(seed=c[2])
        st, _ = _case(orc, scenes, *c, make=lambda sc: RuledOracle(orc, sc, rule), **kw)
        print(st.report())
        assert any(f.startswith(what) for f in st.failures), (name, c, st.failures[:4])


def test_mutant_populations_swapped(orc, scenes):
    """the populations' winners rotated by one: every population steps its real agent with another's winner"""
    st, rs, best = _pops(orc, scenes, 65, mix=lambda b: b[1:] + b[:1])
    print(st.report())
    assert sum("best index" in f for f in st.failures) == 3, st.failures[:6]


def test_mutant_min_obs_dist_from_population_0(orc, scenes):
    """every population's safe-distance term computed from population 0's min_obs_dist"""
    st, rs, best = _pops(orc, scenes, 65, min_obs_of=lambda p: 0)
    print(st.report())
    assert any(f.startswith("cost[") for f in st.failures), st.failures[:6]
    # min_obs_dist differs between the agents of these populations, or the term could not tell
    assert sum(f.startswith("cost[") for f in st.failures) > 65, len(st.failures)
