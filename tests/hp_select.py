"""Designed selections: populations built so that CfManager::evaluateAgents' argmin and 0.9 hysteresis
(B/src/cf_manager.cpp:335-355) land on chosen agent indices, every one of them decided by the high-precision reference
(tests/hp_reference.py) from the paths the planner returned, and shadowed in full (tests/hp_shadow.py): every agent's
cost, the selected index, the type and random vectors that reach the real agent's step.

A planner's manager step maps agents onto lanes, slots and passes (csrc/pmaf_k_misc.hip k_manager: agent a sits in lane
a % 64, slot (a / 64) % 4 of pass a / 256); the layouts below put exact ties, the only minimum and the stored best
agent where that mapping, its padding and its reduction could go wrong. Exact ties are made with duplicates: agent
`dst` gets agent `src`'s type, gains and random vectors, its rollout is bit-identical to `src`'s, and hp.select_best's
`keys` recognise the tie. Agents are independent of each other, so duplicating or swapping agents leaves every other
agent's cost as the probe (a pass without duplicates, ranked by the reference) found it.

Reads planners only through the object handed to it: imports neither oracle/ nor the package (tests/test_hp_reference.py
checks this with `ast`); the scenes module is passed in.
"""
import numpy as np

import hp_reference as hp
import hp_shadow as sh

# the five heuristics without Had (its rotation vector divides by a cross product's norm unguarded)
FIVE = (hp.GOAL, hp.OBSTACLE, hp.GOAL_OBSTACLE, hp.VEL, hp.RANDOM)
TYPE_P = (0.15, 0.15, 0.15, 0.15, 0.4)
# With a scene's own cost gains (100, 10, 0.001, 1) the costs of a short rollout lie within 2 % of each other and
# `cm < 0.9 cb` never fires. These gains make the workspace term dominate: with xmax at the median final x about half
# of the agents pay (300 (x - xmax))^2 per point beyond it, which spreads the costs over +-20 %. The safe-distance gain
# is small but not 0: k_safe / min_obs_dist (0.003 .. 0.03 here, against rounding bounds of 1e-15) brings every agent's
# min_obs_dist into its compared cost, so a planner that takes it from another agent, slot or population fails.
COST_GAINS = np.array([1.0, 1.0, 1e-3, 300.0])
START_VEL = np.array([0.05, 0.0, 0.0])
GAIN_KEYS = ("k_attr", "k_circ", "k_damp", "k_repel")
ROLLOUT_MAX_UNDECIDABLE = 0.10     # K-step rollouts from the reset state, as in tests/test_hp_reference.py


def selection_scene(scenes, N, seed, dups=(), horizon=6, M=24, **over):
    """a synthetic scene of M moving spheres with explicit agent types (the five non-Had heuristics) and every agent
    its own gains, so that costs are pairwise distinct. dups: (dst, src) pairs -- agent dst gets the type, gains and
    random vectors agent src had BEFORE any pair was applied (so (a, b), (b, a) swaps two agents). over: scene entries
    replaced before the pairs are applied (goal, agent_types, cost_gains, ws_limits, ...)"""
    sc = scenes.synthetic_scene(N, horizon, M, config_id=11, scene_id=seed, dynamic=True)
    rng = np.random.default_rng(4000 + seed)
    sc["agent_types"] = rng.choice(FIVE, N, p=TYPE_P).astype(np.int32)
    sc["k_attr"] = rng.uniform(3.0, 5.0, N)
    sc["k_circ"] = rng.uniform(0.015, 0.035, N)
    sc["k_damp"] = rng.uniform(2.5, 4.0, N)
    sc["k_repel"] = rng.uniform(0.05, 0.1, N)
    sc["random_vecs"] = np.array(sc["random_vecs"], dtype=np.float64)
    sc["cost_gains"] = COST_GAINS.copy()
    sc.update(over)
    keys = GAIN_KEYS + ("agent_types", "random_vecs")
    orig = {k: np.array(sc[k]) for k in keys}
    for k in keys:
        sc[k] = orig[k].copy()
    for dst, src in dups:
        for k in keys:
            sc[k][dst] = orig[k][src]
    return sc


def _scs(scene):
    return [scene] if isinstance(scene, dict) else list(scene)


def _snap(planner, P):
    s = sh.snapshot(planner)
    return [s] if P == 1 else s


def prepare(planner, scene):
    """every agent reset to the start with START_VEL and rolled out, independently of any agent's gains (a first tick
    would move the real agent with agent 0's). init_pos 0.25 m from the start: the step's gate is open. Returns the
    per-population init_pos [P, 3]"""
    scs = _scs(scene)
    one = len(scs) == 1
    starts = np.stack([s["start"] for s in scs])
    ip = starts + np.array([0.0, 0.0, -0.25])
    obs = np.stack([s["obstacles"] for s in scs])
    planner.set_initial_position(ip[0] if one else ip)
    planner.set_real_position(starts[0] if one else starts)
    planner.reset_agents(starts[0] if one else starts, START_VEL if one else np.tile(START_VEL, (len(scs), 1)),
                         obs[0] if one else obs)
    planner.rollout()
    return ip


class Probe:
    """the reference's ranking of a prepared population without duplicates: costs (floats of the reference values),
    order (ascending), w (the argmin hp.select_best decides), ws_limits (xmax at the median final x)"""

    def __init__(self, w, costs, order, ws_limits):
        self.w, self.costs, self.order, self.ws_limits = w, costs, order, ws_limits


def spread_ws_limits(scene, snap):
    """the scene's workspace limits with xmax at the median final x of the prepared rollouts"""
    n = snap["n"]
    ws = np.array(scene["ws_limits"], dtype=np.float64)
    ws[0] = float(np.median(snap["paths"][np.arange(len(n)), n - 1, 0]))
    return ws


def probe(planner, scene, A):
    """rank a throw-away planner's prepared population by the reference: the handle's own choice is not consulted.
    Sets scene["ws_limits"] (spread_ws_limits) unless the scene carries `fixed_ws`"""
    prepare(planner, scene)
    snap = sh.snapshot(planner)
    if not scene.get("fixed_ws"):
        scene["ws_limits"] = spread_ws_limits(scene, snap)
    N = int(scene["n_agents"])
    A.seen = {}
    q = [hp.agent_cost(A, snap["paths"][i, :snap["n"][i]], snap["min_obs_dist"][i], scene["goal"],
                       scene["approach_dist"], scene["cost_gains"], scene["ws_limits"]) for i in range(N)]
    w = hp.select_best(A, q, 0)
    c = np.array([x.f for x in q])
    return Probe(w, c, [int(i) for i in np.lexsort((np.arange(N), c))], scene["ws_limits"])


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
TIES = ("plain", "next_slot", "next_pass", "last", "lane_order", "all_same", "tail")
PRIORS = ("keep_dup", "keep_near", "switch", "switch_far")


def has_room(kind, N, where=None):
    """whether population size N has room for the layout (and, for the hysteresis layouts, the prior position)"""
    if kind in ("plain", "all_same", "zero"):
        return where is None or _prior_index(N, where) is not None
    if kind == "next_slot":
        return N >= 65
    if kind == "next_pass":
        return N >= 257
    if kind in ("last", "tail"):
        return N >= 2
    if kind == "lane_order":
        return N >= 129
    if kind == "switch_far":
        return N >= 129 and where in ("mid", "high") and _prior_index(N, where) is not None
    if kind in PRIORS:
        return N >= 2 and _prior_index(N, where) is not None
    raise ValueError(kind)


def _prior_index(N, where):
    """the stored best agent's index: 'mid' in 64..255, 'high' at 256 or above, 'last' N - 1"""
    if where == "mid":
        return 100 if N > 100 else (64 if N > 64 else None)
    if where == "high":
        return 300 if N > 300 else (256 if N > 256 else None)
    if where == "last":
        return N - 1 if N >= 2 else None
    raise ValueError(where)


def cm_of(pr):
    return pr.costs[pr.w]


def design(kind, N, pr, where=None):
    """dict(dups, prior, expect): the duplicate pairs, the stored best agent's index (None: has_best = 0) and the index
    the selection must return, by construction. pr: the Probe of the same (N, seed) without duplicates"""
    src = list(range(N))                     # src[i]: the probe agent whose type, gains and random vectors agent i gets
    if kind == "all_same":
        return dict(dups=[(i, 0) for i in range(1, N)], prior=None, expect=0)
    if kind == "zero":
        j = None if where is None else _prior_index(N, where)
        return dict(dups=[], prior=j, expect=0 if j is None else j)
    w = pr.w

    def swap(i, j):
        src[i], src[j] = src[j], src[i]

    at = None
    if kind == "next_slot":                  # winner and its copy in the same lane, one slot on
        at = min(5, N - 65)
        swap(at, w)
        src[at + 64] = w
    elif kind == "next_pass":                # ... the same lane and slot, one pass on
        at = min(5, N - 257)
        swap(at, w)
        src[at + 256] = w
    elif kind == "last":                     # ... at N - 1
        at = min(5, N - 2)
        swap(at, w)
        src[N - 1] = w
    elif kind == "lane_order":
        # the lower copy (70: lane 6, slot 1) in a higher lane than the upper one (130: lane 2; 128: lane 0): the lanes'
        # first minima are 70 and 130, and only the index rule of the cross-lane reduction returns 70
        hi = 130 if N > 130 else 128
        swap(70, w)
        src[hi] = w
    elif kind == "tail":                     # the only minimum in the last, partly filled group of lanes
        swap(N - 1, w)
    elif kind in PRIORS:
        j = _prior_index(N, where)
        if kind == "switch_far":             # the argmin itself at 64 or above (70: lane 6, slot 1), and only there
            swap(70, w)
        elif w in (j, j % 64):               # keep the argmin's own agent clear of the designed positions
            swap(next(i for i in range(N) if i not in (j, j % 64)), w)
        near = [i for i in pr.order[1:] if pr.costs[i] * 0.95 <= cm_of(pr) and pr.costs[i] > cm_of(pr) * (1.0 + 1e-9)]
        cm = pr.costs[w]
        worst = pr.order[-1]
        if not cm < 0.85 * pr.costs[worst]:
            raise ValueError("no agent decidedly above cm / 0.9: choose another seed or other gains")
        if kind == "keep_dup":               # the stored best ties with the argmin: cm < 0.9 cm is false, it stays
            other = worst
            src[j] = w
        elif kind == "keep_near":            # the stored best costs a little more than the argmin: it stays
            if not near:
                raise ValueError("no agent within 5 % above the minimum: choose another seed")
            other = worst
            src[j] = near[-1]
        elif kind == "switch":               # the stored best costs far more: the selection switches to the argmin
            other = w
            src[j] = worst
        else:                                # ... and both s_cost[min_idx] and s_cost[id - 1] are read at 64 or above
            if not near:
                raise ValueError("no agent within 5 % above the minimum: choose another seed")
            other = near[-1]                 # (a cost the argmin does not undercut by 10 %: read instead, it would keep)
            src[j] = worst
            src[70 % 64] = worst             # (and so would s_cost[min_idx % 64] read for the argmin's cost)
        if j >= 64:                          # the agent a `cost[(id - 1) % 64]` would read instead decides the other way
            src[j % 64] = other
    elif kind != "plain":
        raise ValueError(kind)
    dups = [(i, s) for i, s in enumerate(src) if s != i]
    argmin = min(i for i, s in enumerate(src) if s == w)
    if kind in PRIORS:
        return dict(dups=dups, prior=j, expect=argmin if kind in ("switch", "switch_far") else j)
    return dict(dups=dups, prior=None, expect=argmin)


# ---------------------------------------------------------------------------------------------------------------------
# the shadowed pass
# ---------------------------------------------------------------------------------------------------------------------
def run_selection(planner, scene, A, st, prior=None, entry="tick", n_rollouts=4, rollout_stats=None):
    """prepare the population(s), install `prior` (an index, or one per population; None: no stored best agent) with
    set_best, then one `tick` or one stand-alone `evaluate` (followed by move_real with the returned index), shadowed:
    every agent's cost and the selection (check_evaluate with all agents), best_type against the scene's agent types,
    the real agent's step with the selected agent's gains, type and random vectors (check_real) and, after a tick, the
    rollouts of n_rollouts sampled agents (into rollout_stats). Returns the selected indices, one per population."""
    scs = _scs(scene)
    P, s0 = len(scs), scs[0]
    one = P == 1
    N = int(s0["n_agents"])
    obs = np.stack([s["obstacles"] for s in scs])
    types = [sh.agent_types(s) for s in scs]
    ip = prepare(planner, scene)
    pr = None
    if prior is not None:
        pr = [int(prior)] * P if np.ndim(prior) == 0 else [int(j) for j in prior]
        planner.set_best(np.array([j + 1 for j in pr], dtype=np.int32),
                         np.array([types[p][pr[p]] for p in range(P)], dtype=np.int32),
                         np.stack([scs[p]["random_vecs"][pr[p]] for p in range(P)]))
    pre = _snap(planner, P)
    for p in range(P):
        assert pre[p]["best_id"] == (pr[p] + 1 if pr else 0), (p, pre[p]["best_id"])
    if entry == "tick":
        best = planner.tick(obs[0] if one else obs, s0["dt"], s0["cost_gains"], s0["ws_limits"])
    else:
        best = planner.evaluate(s0["cost_gains"], s0["ws_limits"])
        planner.move_real(obs[0] if one else obs, s0["dt"], 1, int(best) if one else np.asarray(best, dtype=np.int32))
    best = [int(b) for b in np.ravel(best)]
    post = _snap(planner, P)
    sample = sorted(np.random.default_rng(N).choice(N, min(N, n_rollouts), replace=False).tolist())
    for p, sc in enumerate(scs):
        tag = "" if one else "pop %d " % p
        assert post[p]["best_id"] == best[p] + 1, (p, post[p]["best_id"], best[p])
        sh.check_evaluate(A, st, sc, pre[p], post[p]["costs"], best[p], range(N))
        st.expect(tag + "best_type", types[p][best[p]], int(post[p]["best_type"]))
        sh.check_real(A, st, sc, pre[p], post[p], ip[p], obs[p], best[p])
        if entry == "tick" and rollout_stats is not None:
            sh.check_rollouts(A, rollout_stats, sc, post[p]["real_pos"], post[p]["real_vel"], post[p]["real_known"],
                              pre[p]["rot_vecs"], pre[p]["success"], post[p], obs[p], ip[p], sample)
    return best


_PROBES = {}


def probed(make_planner, scenes, N, seed, A, key, **over):
    """the Probe of (N, seed) on a throw-away planner from make_planner(scene); cached per `key` (the planner kind: its
    paths, and so the ranking's inputs, are that kind's)"""
    k = (key, N, seed, tuple(sorted((a, repr(b)) for a, b in over.items())))
    if k not in _PROBES:
        sc = selection_scene(scenes, N, seed, **over)
        pl = make_planner(sc)
        try:
            _PROBES[k] = probe(pl, sc, A)
        finally:
            pl.close()
    return _PROBES[k]


def designed_case(make_planner, scenes, N, seed, kind, A, st, key, where=None, entry="tick", rollout_stats=None,
                  inspect=None, **over):
    """probe (cached), lay out `kind`, run the designed pass in full and hold the selection to the layout's index.
    inspect(planner, scene, best): called before the planner is closed. Returns (scene, best index)"""
    if kind == "zero":
        # every cost exactly 0 (only the workspace gain, no point outside the limits): 0 < 0.9 * 0 is false, 0 <= 0 true
        over = dict(over, cost_gains=np.array([0.0, 0.0, 0.0, 1.0]), ws_limits=np.array([9.0, -9.0, 9.0, -9.0, 9.0, -9.0]))
        pr = None
    elif kind == "all_same" or N == 1:
        pr = None
    else:
        pr = probed(make_planner, scenes, N, seed, A, key, **over)
        over = dict(over, ws_limits=pr.ws_limits)
    d = design(kind, N, pr, where) if N > 1 else dict(dups=[], prior=None, expect=0)
    sc = selection_scene(scenes, N, seed, dups=d["dups"], **over)
    pl = make_planner(sc)
    try:
        if pr is None and kind != "zero":
            prepare(pl, sc)
            sc["ws_limits"] = spread_ws_limits(sc, sh.snapshot(pl))
        best = run_selection(pl, sc, A, st, prior=d["prior"], entry=entry, rollout_stats=rollout_stats)[0]
        if inspect is not None:
            inspect(pl, sc, best)
    finally:
        pl.close()
    assert best == d["expect"], "%s N=%d: selected %d, the layout puts it at %d\n%s" % (kind, N, best, d["expect"],
                                                                                       st.report())
    return sc, best


# ---------------------------------------------------------------------------------------------------------------------
# the designed cases, shared by the oracle test (tests/test_hp_select.py) and the kernel test
# (tests/test_hp_select_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
# the smallest sizes at which each path of a four-agents-per-lane, 256-agents-per-pass manager exists: one agent; one
# short of, exactly and one past a wave (slot 1 appears); 129 (slot 2); one short of, exactly and one past a pass; 321
# (the second pass's slot 1, lane 0 alone in it); 577 (a third pass)
SIZES = (1, 63, 64, 65, 129, 255, 256, 257, 321, 577)
SEED = 0

TIE_CASES = [(N, kind) for N in SIZES for kind in TIES if (N > 1 or kind == "plain") and has_room(kind, N)]
# (N, layout, where the stored best agent sits)
PRIOR_CASES = [(129, "keep_dup", "mid"), (129, "switch", "mid"), (255, "keep_near", "mid"),
               (321, "keep_dup", "high"), (321, "keep_near", "high"), (321, "switch", "high"),
               (577, "switch", "high"), (577, "keep_dup", "last"), (65, "keep_dup", "last"), (257, "switch", "last"),
               (63, "keep_near", "last"), (129, "zero", "mid"), (129, "switch_far", "mid"),
               (321, "switch_far", "high")]
# the stand-alone evaluate (a manager launch that only selects)
EVALUATE_CASES = [(65, "tail", None), (321, "lane_order", None), (321, "switch", "high"), (577, "next_pass", None),
                  (257, "keep_dup", "high")]


# (N, layout, seed): populations whose winner is a Random agent while agent 0 is not, and in whose field the real agent
# latches rotation vectors in its step -- a Random agent's come from its random vectors, so the winner's type AND its
# random vectors, copied from index N - 1 or 70, are visible in the compared real step
RECORD_CASES = [(257, "tail", 1), (321, "lane_order", 1)]


def case_id(N, kind, where=None, entry="tick"):
    return "%s%s@%d%s" % (kind, "-" + where if where else "", N, "" if entry == "tick" else "-" + entry)


def near_goal(scenes):
    """a goal 0.2535 m from the start: within the 6-step horizon some agents come inside approach_dist (0.25), where the
    goal-distance term of the cost is dropped, and some do not"""
    s = scenes.synthetic_scene(1, 1, 1)
    return dict(goal=s["start"] + np.array([0.2535, 0.0, 0.0]))


def population_scenes(scenes, N, seeds=(0, 1, 2)):
    """P scenes for one handle: different obstacle fields, random vectors, gains and goals; the agent types are the
    first scene's (a handle holds one type table for all its populations)"""
    goals = [np.array([0.6, 0.0, 0.7]), np.array([0.5, 0.3, 0.9]), np.array([0.55, -0.3, 0.5])]
    s0 = selection_scene(scenes, N, seeds[0])
    out = [s0]
    for k, s in enumerate(seeds[1:], 1):
        out.append(selection_scene(scenes, N, s, goal=goals[k % 3], agent_types=s0["agent_types"]))
    return out


def run_populations(planner, scs, A, st, entry="tick", rollout_stats=None):
    """P populations in one handle, workspace xmax at the median final x over all of them; returns the winners"""
    prepare(planner, scs)
    snaps = _snap(planner, len(scs))
    ws = np.array(scs[0]["ws_limits"], dtype=np.float64)
    ws[0] = float(np.median([s["paths"][np.arange(len(s["n"])), s["n"] - 1, 0] for s in snaps]))
    for s in scs:
        s["ws_limits"] = ws
    return run_selection(planner, scs, A, st, entry=entry, rollout_stats=rollout_stats)


def assert_decided(st, rs, n_agents, n_selections=1):
    """all costs compared, every selection compared, nothing undecidable (cap 0)"""
    rs.assert_ok(ROLLOUT_MAX_UNDECIDABLE, min_compared=0)
    st.assert_ok(max_undecidable=0.0)
    assert st.undecidable == 0, st.report()
    assert st.selections == n_selections, st.report()
    assert st.compared == n_selections * (n_agents + 2), st.report()      # costs + selection + real step, per population
