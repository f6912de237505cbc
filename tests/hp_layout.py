"""Designed obstacle layouts: scenes built so that the rollout kernels' per-obstacle reductions -- the closest obstacle
of attractorForceScaling (B/src/cf_agent.cpp:195-227), the nearest other obstacle of the Obstacle / GoalObstacle latch
(:434-446, :480-492), the list of non-zero circular terms (:72-108) and min_obs_dist_ -- land on chosen obstacle
indices, every one of them decided by the high-precision reference (tests/hp_reference.py) and shadowed in full
(tests/hp_shadow.py). tests/hp_select.py does the same along the agent axis of the manager step.

Where an obstacle index lives (read from csrc/; M field obstacles, the trailing repulsive one is not in these sweeps):
  k_rollout_w64 (pmaf_k_w64.hip, pmaf_rollout_w64.hpp)   obstacle i in lane i % 64, slot i / 64; one slot for M <= 60,
                                                         2 slots for M = 61..128, 3 to 192, 4 to 256 (pmaf_route.hpp
                                                         route: slots64)
  k_rollout_mw (pmaf_k_mw.hip, base = w * per)           W = max(2, ceil(M / 64)) waves (PMAF_MW raises it, up to 4),
                                                         per = ceil(M / W); obstacle i in wave i / per, lane i % per
  k_rollout_grp / generic k_rollout (i = t * LPA + sub)  obstacle i in lane i % LPA of the agent's group, slot i / LPA;
                                                         64 / LPA agents per wave
The layouts below put exact ties, the only candidate, the term holders and the latching obstacles on the two sides of
those boundaries. Unnamed field obstacles sit on a line more than 200 m away and 128 m apart: out of every shell and
beyond the latch's 100 m horizon.

Exact geometry: every signed permutation of (0.1875, 0.25, 0) has squared norm 0.09765625 and norm 0.3125 exactly under
both dot associations, axis offsets of 0.25 and 100 have exact norms, and all radii are 0.0625, so the strict policies
compute the tied distances without a rounding and the reference decides the tie with bound 0.

Reads planners only through the object handed to it: imports neither oracle/ nor the package (tests/test_hp_reference.py
checks this with `ast`).
"""
import numpy as np

import hp_reference as hp
import hp_shadow as sh

P0 = np.array([0.25, 0.25, 0.5])
V0 = np.array([0.125, 0.0, 0.0])
# the term-list cases also run under the contracted policy, whose root is not correctly rounded: there the reference
# cannot decide the gate's speed test at V0 (|V0| = 0.5 vel_max exactly). They start at VC, 0.75 vel_max, instead
VC = np.array([0.1875, 0.0, 0.0])
INIT = P0 - np.array([0.0, 0.0, 0.5])            # 0.5 m from the start: the step's gate is open
GOAL = P0 + np.array([1.0, 0.125, 0.0625])       # off every mirror plane of the tied offsets: their g.ro all differ
DT, SHELL, RAD, ORAD = 0.0625, 0.375, 0.0625, 0.0625
SENTINEL = [100.0, 100.0, 100.0, 0.0, 0.0, 0.0, 0.1]
ALL_TYPES = (hp.HAD, hp.GOAL, hp.OBSTACLE, hp.GOAL_OBSTACLE, hp.VEL, hp.RANDOM)
LATCH_TYPES = (hp.OBSTACLE, hp.GOAL_OBSTACLE, hp.GOAL)
# tied offsets from the agent (norm 0.3125, surface distance 0.1875); pairwise centre distances all different
TIED = (np.array([0.1875, 0.25, 0.0]), np.array([0.25, 0.1875, 0.0]), np.array([0.1875, 0.0, 0.25]))
BEHIND = np.array([-0.25, 0.0, 0.0])             # surface distance 0.125; ro.g < 0 and ro.v = -0.03125 < -0.01: skipped
ENTER = np.array([0.25, 0.0625, 0.0])            # the latching obstacle; with NEIGH, four different distances to the agent
ENTER_B = np.array([0.125, -0.25, 0.1875])       # a second one, latching in the same step
# tied offsets from a latching obstacle (centre distance 0.25, as in tests/hp_edges.py E_CLOSEST); pairwise distances
# sqrt(1/8), 1/2, sqrt(1/8), so the neighbours' own latches meet no tie -- and ENTER_B's are others than ENTER's
NEIGH = (np.array([0.25, 0.0, 0.0]), np.array([0.0, 0.25, 0.0]), np.array([0.0, -0.25, 0.0]))
NEIGH_B = (np.array([0.0, 0.0, 0.25]), np.array([0.0, 0.0, -0.25]))


def far_row(i):
    return [256.0 + 128.0 * i, 16.0, 8.0, 0.0, 0.0, 0.0, ORAD]


def row(offset, vel=(0.0, 0.0, 0.0), origin=P0):
    return list(np.asarray(origin) + np.asarray(offset)) + list(vel) + [ORAD]


def layout_scene(M, named, types=ALL_TYPES, cap=2, n_agents=None, **over):
    """M field obstacles + the sentinel; named: {index: row}. n_agents: the types repeated to that many agents"""
    rows = [far_row(i) for i in range(M)]
    for i, r in named.items():
        assert 0 <= i < M, (i, M)
        rows[i] = list(r)
    rows.append(SENTINEL)
    n = len(types) if n_agents is None else n_agents
    types = [types[a % len(types)] for a in range(n)]
    rng = np.random.default_rng(3)
    rv = rng.uniform(-1, 1, (n, M + 1, 3))
    rv /= np.linalg.norm(rv, axis=-1, keepdims=True)
    s = dict(name="layout", n_agents=n, max_prediction_steps=cap, dt=DT, velocity_max=0.25, approach_dist=0.25,
             detect_shell_rad=SHELL, agent_mass=1.0, radius=RAD, k_attr=4.0, k_circ=0.03125, k_repel=0.0625,
             k_damp=4.0, cost_gains=np.array([100.0, 10.0, 0.001, 1.0]),
             ws_limits=np.array([1.0, -1.0, 1.0, -1.0, 2.0, 0.0]), start=P0.copy(), goal=GOAL.copy(),
             obstacles=np.asarray(rows, dtype=np.float64), random_vecs=rv, agent_types=np.asarray(types, dtype=np.int32))
    s.update(over)
    return s


class Mapping:
    """one planner family at one obstacle count: the environment and lanes_per_agent that select it, the launch
    configuration it must report, and unit(i) = the slot (wave, for k_rollout_mw) obstacle i lives in"""

    def __init__(self, key, M, kind, env=None, lpa=0, n_agents=6, waves=1, per=0, sliced=False, light=False, families="ABC"):
        self.key, self.M, self.kind, self.env, self.lpa, self.n_agents = key, M, kind, dict(env or {}), lpa, n_agents
        self.waves, self.per, self.light, self.families = waves, per, light, families
        self.width = per if kind == "mw" else (lpa or 64)
        self.expect = dict(lanes_per_agent=lpa or 64, waves_per_agent=waves, priority_slices=sliced)
        if kind == "mw":
            self.expect["obstacles_per_wave"] = per

    def unit(self, i):
        return i // self.width

    def lane(self, i):
        return i % self.width

    @property
    def units(self):
        return (self.M + self.width - 1) // self.width


def _mw(M, forced=None, light=False):
    W = max(2, (M + 63) // 64)
    env = {}
    if forced is not None:
        assert forced >= W
        W, env = forced, {"PMAF_MW": str(forced)}
    return Mapping("mw-W%d-M%d%s" % (W, M, "" if forced is None else "-forced"), M, "mw", env, waves=W, per=(M + W - 1) // W,
                   light=light)


W64_ONE = Mapping("w64-one-slot-M60", 60, "w64")
# (the LDS-batch force sum differs from the default kernel in the term list alone: no latch cases)
W64_ONE_LDS = Mapping("w64-one-slot-lds-M60", 60, "w64", {"PMAF_SUM": "lds"}, families="AC")
W64_TILES = [Mapping("w64-tiles-M%d" % m, m, "w64", {"PMAF_MW": "0"}) for m in (70, 128, 200, 256)]
MW_FORCED = [_mw(100, 2), _mw(100, 3), _mw(100, 4), _mw(183, 4)]
# (the default rule's wave counts and splits: every tie set; of families B and C the cases at the wave boundaries)
MW_DEFAULT = [_mw(m, light=True) for m in (61, 122, 123, 183, 184, 244, 245, 256)]
GRP = [Mapping("grp-%dx2" % l, 2 * l, "grp", lpa=l, n_agents=n) for l, n in ((8, 12), (16, 6), (32, 7))]
GENERIC = [Mapping("generic-64-M128", 128, "generic", {"PMAF_FORCE_GENERIC": "1"}, lpa=64),
           Mapping("generic-16-M32", 32, "generic", {"PMAF_FORCE_GENERIC": "1"}, lpa=16)]
MAPPINGS = [W64_ONE, W64_ONE_LDS] + W64_TILES + MW_FORCED + MW_DEFAULT + GRP + GENERIC
BY_KEY = {m.key: m for m in MAPPINGS}


def tie_sets(mp):
    """index sets of the exact ties for a mapping, the order giving the tied offsets (TIED[0] to the first index, ...):
    the winner is the LOWEST index, and each set puts it where a lane-major, slot-major or wave-major rule finds another"""
    M, w = mp.M, mp.width
    if mp.kind == "w64" and M <= 60:
        return [(0, 59), (59, 0), (31, 32)]
    if mp.kind == "mw":
        s = [(u * w - 1, u * w) for u in range(1, mp.units)]             # the two sides of every wave boundary
        s.append(((mp.units - 1) * w + 1, w - 2))                          # low lane of the last wave, high lane of wave 0
        s.append((M - 1, 0))
        if mp.units >= 3:
            s.append((2 * w + 3, w + 20, 40 % w))                          # three waves
        return s
    if mp.kind == "grp" or w < 64:
        # slot 1 of lane 1 against slot 0 of lane 5, slot 1 of lane 5 against slot 0 of lane 1, the slot boundary, the ends
        return [(w + 1, 5), (w + 5, 1), (w - 1, w), (M - 1, 0), (w + 2, w - 2, 3)]
    s = [(69, 10), (5, 67), (63, 64), (M - 1, 0)]
    if M > 128:
        s += [(127, 128), (130, 2 * 64 + 1, 3 * 64)]
    return [t for t in s if max(t) < M]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """a scene, the state every agent is reset to, and `pre(A, case, counts)`: the case's own precondition, re-evaluated
    in the reference (counts: per agent, the number of circular terms the reference produced in each step)"""

    def __init__(self, name, family, mp, scene, pre, vel=V0, info=None):
        self.name, self.family, self.mp, self.scene, self.pre, self.vel = name, family, mp, scene, pre, np.asarray(vel)
        self.info = info or {}
        self.agents = list(range(int(scene["n_agents"])))     # the shadowed agents (`cases` thins them at large M)
        self.pos, self.init = P0, INIT

    @property
    def steps(self):
        return int(self.scene["max_prediction_steps"]) - 1


class TermCounts:
    """records how many terms hp.circ_terms returned, call by call, while a rollout is shadowed"""

    def __enter__(self):
        self.counts, self._orig = [], hp.circ_terms

        def rec(*a, **k):
            t = self._orig(*a, **k)
            self.counts.append(len(t))
            return t
        hp.circ_terms = rec
        return self

    def __exit__(self, *exc):
        hp.circ_terms = self._orig


class Falsified:
    """a planner that is handed mutate(obstacle rows) at its reset while the shadow keeps the true rows (mutants)"""

    def __init__(self, inner, mutate):
        self.inner, self.mutate = inner, mutate

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def reset_agents(self, pos, vel, obs):
        self.inner.reset_agents(pos, vel, self.mutate(np.array(obs, dtype=np.float64, copy=True)))


def run_case(case, make_planner, A, st, agents=None, mutate=None, check_pre=True):
    """reset every agent to the case's state, roll out case.steps steps, shadowed; then the case's precondition"""
    sc = case.scene
    pl = make_planner(sc)
    n0 = st.compared + st.undecidable
    try:
        drv = pl if mutate is None else Falsified(pl, mutate)
        drv.set_initial_position(case.init)
        with TermCounts() as tc:
            sh.shadow_reset_rollout(drv, sc, case.pos, case.vel, sc["obstacles"], case.init, A, st,
                                    case.agents if agents is None else agents)
    finally:
        pl.close()
    n = st.compared + st.undecidable - n0
    counts = None
    if len(tc.counts) == n * case.steps:
        counts = [tc.counts[a * case.steps:(a + 1) * case.steps] for a in range(n)]
    if check_pre:
        case.pre(A, case, counts)
    return counts


def _agent(A, sc):
    return hp.Agent(A, P0, V0, sc["goal"], INIT, [False] * len(sc["obstacles"]), np.zeros((len(sc["obstacles"]), 3)),
                    atype=hp.GOAL, **sh._params(sc))


def _dist(A, sc, i):
    return hp._floored_dist(A, A.v3(P0), hp.obstacles_from_rows(A, sc["obstacles"])[i], A.c(RAD))


def _skipped(A, sc, i, vel=V0):
    o = hp.obstacles_from_rows(A, sc["obstacles"])[i]
    ro = A.vsub(o.pos, A.v3(P0))
    g = A.vsub(A.v3(sc["goal"]), A.v3(P0))
    return (A.decide("skip_dir", A.dot(A.normalized(ro), A.normalized(g)), "<", A.c(-0.01)) and
            A.decide("skip_vel", A.dot(ro, A.vsub(A.v3(vel), o.vel)), "<", A.c(-0.01)))


def _others_farther(A, sc, idxs, d):
    for i in range(len(sc["obstacles"]) - 1):
        if i not in idxs:
            assert A.decide("pre", _dist(A, sc, i), ">", d), i


# -- family A --------------------------------------------------------------------------------------------------------
def tie_case(mp, idxs):
    """exact tie of attractorForceScaling's closest obstacle at `idxs`, all unskipped: min(idxs) enters w2"""
    sc = layout_scene(mp.M, {i: row(TIED[k]) for k, i in enumerate(idxs)}, n_agents=mp.n_agents)

    def pre(A, case, counts):
        d = [_dist(A, sc, i) for i in idxs]
        assert all(q.e == 0.0 and q.v == A.c(0.1875).v for q in d), d
        _others_farther(A, sc, idxs, d[0])
        assert not any(_skipped(A, sc, i) for i in idxs)
        assert counts is not None and all(c == [len(idxs)] for c in counts), counts
    return Case("%s tie %s" % (mp.key, "=".join(map(str, idxs))), "A", mp, sc, pre, info=dict(idxs=idxs))


def skipped_closest_case(mp, s, u):
    """obstacle s behind the agent (skipped by circForce, so not in min_obs_dist_) strictly closer than the only
    unskipped one, u: the scaling's w1 and w2 come from s, min_obs_dist from u"""
    sc = layout_scene(mp.M, {s: row(BEHIND), u: row(TIED[0])}, n_agents=mp.n_agents)

    def pre(A, case, counts):
        assert _skipped(A, sc, s) and not _skipped(A, sc, u)
        assert A.decide("pre", _dist(A, sc, s), "<", _dist(A, sc, u))
        _others_farther(A, sc, (s, u), _dist(A, sc, u))
        assert counts is not None and all(c == [1] for c in counts), counts
    return Case("%s skipped closest %d, unskipped %d" % (mp.key, s, u), "A", mp, sc, pre, info=dict(s=s, u=u))


def behind_unskipped_case(mp, s, u):
    """the obstacle behind the agent overtakes it (0.25 m/s along x: ro.rel_vel = +0.03125), so circForce does NOT skip
    it: the closest obstacle, min_obs_dist and a term all come from s"""
    sc = layout_scene(mp.M, {s: row(BEHIND, vel=(0.25, 0.0, 0.0)), u: row(TIED[0])}, n_agents=mp.n_agents)

    def pre(A, case, counts):
        assert not _skipped(A, sc, s) and not _skipped(A, sc, u)
        assert A.seen["skip_dir"] == {True, False} and A.seen["skip_vel"] == {False}, A.seen
        assert A.decide("pre", _dist(A, sc, s), "<", _dist(A, sc, u))
        assert counts is not None and all(c == [2] for c in counts), counts
    return Case("%s overtaking obstacle %d behind, %d ahead" % (mp.key, s, u), "A", mp, sc, pre, info=dict(s=s, u=u))


def only_case(mp, i):
    """the only obstacle inside the shell at index i"""
    sc = layout_scene(mp.M, {i: row(TIED[1])}, n_agents=mp.n_agents)

    def pre(A, case, counts):
        assert A.decide("pre", _dist(A, sc, i), "<", A.c(SHELL))
        _others_farther(A, sc, (i,), A.c(SHELL))
        assert counts is not None and all(c == [1] for c in counts), counts
    return Case("%s only obstacle %d" % (mp.key, i), "A", mp, sc, pre, info=dict(i=i))


def family_a(mp):
    M, w = mp.M, mp.width
    hi = (mp.units - 1) * w + min(7, M - 1 - (mp.units - 1) * w)          # a lane of the last slot / wave
    cases = [tie_case(mp, t) for t in tie_sets(mp)]
    cases += [skipped_closest_case(mp, hi, 3), only_case(mp, M - 1)]
    if not mp.light:
        cases += [skipped_closest_case(mp, 2, hi), skipped_closest_case(mp, M - 1, 0), behind_unskipped_case(mp, hi, 3),
                  only_case(mp, 0), only_case(mp, hi)]
    return cases


# -- family B --------------------------------------------------------------------------------------------------------
def latch_case(mp, groups, moving, far100=None, tag=""):
    """groups: [(e, origin offset, [(index, offset from e's obstacle), ...])] -- obstacle e enters the shell and latches,
    its tied nearest others (centre distance 0.25 exactly) sit at the given indices: the lowest wins. moving: one far
    obstacle gets a velocity, which sends every kernel through its cooperative scan (see tests/test_hp_layout_gpu.py).
    far100: (e, n) -- e's only neighbour, n, exactly 100 m away: not accepted (`min_d > d` from 100.0), index 0 stays"""
    named = {}
    for e, off, nb in groups:
        named[e] = row(off)
        for i, o in nb:
            assert i not in named, (i, groups)
            named[i] = row(np.asarray(off) + np.asarray(o))
    if far100:
        named[far100[1]] = row(np.asarray(named[far100[0]][:3]) - P0 + np.array([100.0, 0.0, 0.0]))
    sc = layout_scene(mp.M, named, types=LATCH_TYPES, n_agents=mp.n_agents)
    if moving:
        mv = next(i for i in range(mp.M - 2, -1, -1) if i not in named)
        sc["obstacles"][mv, 3:6] = [0.5, 0.0, -0.25]

    def pre(A, case, counts):
        obs = hp.obstacles_from_rows(A, sc["obstacles"])
        for e, off, nb in groups:
            assert A.decide("pre", _dist(A, sc, e), "<", A.c(SHELL))                 # it latches in this step
            want = min(i for i, _ in nb) if nb else 0
            for i, _ in nb:
                d = A.norm(A.vsub(obs[i].pos, obs[e].pos))
                assert d.e == 0.0 and d.v == A.c(0.25).v, (e, i, d)
            assert hp._closest_other(A, obs, e) == want, (e, want)
        if far100:
            d = A.norm(A.vsub(obs[far100[1]].pos, obs[far100[0]].pos))
            assert d.e == 0.0 and d.v == A.c(100.0).v, d
        assert np.any(sc["obstacles"][:-1, 3:6] != 0.0) == bool(moving)
    name = "%s latch %s%s%s" % (mp.key, " ".join("%d<-%s" % (e, "=".join(str(i) for i, _ in nb) or "none")
                                                 for e, _, nb in groups), tag, " moving" if moving else " at rest")
    return Case(name, "B", mp, sc, pre, info=dict(groups=groups, far100=far100, moving=moving))


def family_b(mp):
    M, w = mp.M, mp.width
    mid = w * (mp.units // 2) if mp.units > 1 else 32                       # a slot / wave boundary
    hi = (mp.units - 1) * w + min(7, M - 1 - (mp.units - 1) * w)
    sets = tie_sets(mp)
    cases = []

    def tied(e, t, moving):
        return latch_case(mp, [(e, ENTER, [(i, NEIGH[j]) for j, i in enumerate(t)])], moving)

    for moving in (False, True):
        # every tie set of the mapping that does not hold the entering obstacle's own index (the split kernel's default
        # sizes: the entering obstacle at the wave boundary only)
        for e in ((mid,) if mp.light else (0, mid, M - 1)):
            for t in sets:
                if e not in t:
                    cases.append(tied(e, t, moving))
        # two obstacles latch in the same step, in different slots / waves, with different tied neighbours
        a, b = (hi, 1) if mp.units > 1 else (40, 1)
        na = [i for i in (M - 2, 4) if i not in (a, b)]
        nbs = [i for i in (6, hi - 3 if mp.units > 1 else 50) if i not in (a, b)]
        cases.append(latch_case(mp, [(a, ENTER, [(i, NEIGH[j]) for j, i in enumerate(na)]),
                                     (b, ENTER_B, [(i, NEIGH_B[j]) for j, i in enumerate(nbs)])], moving, tag=" (two)"))
        if not mp.light:
            cases.append(latch_case(mp, [(hi, ENTER, [])], moving, far100=(hi, 2), tag=" 100 m"))
            cases.append(latch_case(mp, [(hi, ENTER, [])], moving, tag=" alone"))
            cases.append(latch_case(mp, [(0, ENTER, [])], moving, tag=" alone at 0"))
    return cases


# -- family C --------------------------------------------------------------------------------------------------------
def _direction(k):
    """a unit vector of the goal-ward hemisphere (x component >= 0.6), different for every k"""
    rng = np.random.default_rng(900 + k)
    u = np.array([1.0, rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9)])
    return u / np.linalg.norm(u)


def _dyadic(x, bits=16):
    return np.round(np.asarray(x) * 2.0 ** bits) / 2.0 ** bits


def term_case(mp, holders, tag, zero_rel=True):
    """K = len(holders) obstacles inside the shell, unskipped and with non-zero relative velocity, at K distinct surface
    distances 0.0625 + k / 1024 (k < 256), over three steps. With K >= 2 the outermost holder moves away at 4 m/s and has
    left the shell by the second step, and (zero_rel) an obstacle that starts at the agent's velocity sits at an index
    between two holders: no term in the first step, one from the second step on"""
    holders = sorted(holders)
    K = len(holders)
    named = {}
    for k, i in enumerate(holders):
        d = 0.0625 + (k * 255 // max(K - 1, 1)) / 1024.0 if K > 1 else 0.125
        named[i] = row(_dyadic((d + RAD + ORAD) * _direction(i)))
    leaver = zero = None
    if K >= 2:
        leaver = holders[-1]
        named[leaver][3:6] = [4.0, 0.0, 0.0]
        free = [i for i in range(holders[0] + 1, holders[-1]) if i not in named]
        if zero_rel and free:
            zero = free[len(free) // 2]
            named[zero] = row(_dyadic(0.325 * _direction(1000 + zero)), vel=VC)
    sc = layout_scene(mp.M, named, cap=4, n_agents=mp.n_agents)
    want = [K, K - (leaver is not None) + (zero is not None), K - (leaver is not None) + (zero is not None)]

    def pre(A, case, counts):
        assert counts is not None
        assert all(c == want for c in counts), (want, counts)
        if zero is not None:
            o = hp.obstacles_from_rows(A, sc["obstacles"])[zero]
            assert all(x.v == 0 and x.e == 0.0 for x in A.vsub(A.v3(VC), o.vel))
            assert A.decide("pre", _dist(A, sc, zero), "<", A.c(SHELL))
        if leaver is not None:                   # inside at the first step; outside after one advance, wherever the agent went
            assert A.decide("pre", _dist(A, sc, leaver), "<", A.c(SHELL))
            o = hp.obstacles_from_rows(A, sc["obstacles"])[leaver]
            far = A.sub(A.norm(A.vsub(A.vadd(o.pos, A.vscale(A.c(DT), o.vel)), A.v3(P0))), A.c(RAD + ORAD + 0.046875))   # (a step moves the agent 0.041 m at the most)
            assert A.decide("pre", far, ">", A.c(SHELL))
    return Case("%s terms K=%d %s" % (mp.key, K, tag), "C", mp, sc, pre, vel=VC,
                info=dict(holders=holders, leaver=leaver, zero=zero, want=want))


def _spread(K, lo, n, stride):
    """K of the n indices lo .. lo + n - 1, `stride` (coprime to n) apart: the holders' lanes are spread, not a prefix"""
    assert K <= n
    return [lo + (stride * j + 2) % n for j in range(K)]


def ragged_case(mp):
    """different list lengths for neighbouring agents of one wave. Every agent of a population starts at one position,
    so the first step's lists cannot differ; per-agent gains make the second and third differ. No obstacle is inside
    the shell in the first step, so the attractor acts unscaled: with k_damp = 64 an agent with k_attr = 64 accelerates
    towards the goal at 4 m/s^2 and one with k_attr = 1 brakes at 11 m/s^2, which puts them up to 3 cm apart after one
    step. A band of obstacles whose surfaces lie 2^-9 m apart, just outside the shell in the goal's direction, is then
    inside the shell of some agents and outside that of their neighbours"""
    M = mp.M
    n = min(M - 2, 16)
    g = (GOAL - P0) / np.linalg.norm(GOAL - P0)
    named = {}
    for k, i in enumerate(_spread(n, 0, M, 5 if M % 5 else 3)):
        u = g + 0.15 * (_direction(i) - g)
        named[i] = row(_dyadic((SHELL + RAD + ORAD + 0.002 + k / 512.0) * u / np.linalg.norm(u)))
    N = mp.n_agents
    sc = layout_scene(M, named, cap=4, n_agents=N, k_attr=np.array([(64.0, 1.0, 16.0, 4.0)[a % 4] for a in range(N)]),
                      k_damp=np.array([(64.0, 64.0, 32.0)[a % 3] for a in range(N)]))
    per_wave = 64 // mp.width

    def pre(A, case, counts):
        assert counts is not None and len(counts) == N
        assert all(c[0] == 0 for c in counts), counts                       # one start position: no list in the first step
        first = counts[:min(per_wave, N)]
        assert all(first[a][1:] != first[a + 1][1:] for a in range(len(first) - 1)), first   # neighbours of one wave differ
        assert max(c[1] for c in first) >= 4 and min(c[1] for c in first) == 0, first
    c = Case("%s ragged lists" % mp.key, "C", mp, sc, pre, vel=VC, info=dict(holders=sorted(named)))
    c.all_agents = True
    return c


def family_c(mp):
    M, w = mp.M, mp.width
    cases = []
    if mp.kind == "w64" and M <= 60:
        # (K thinned for the CPU cost of the reference: of 7 / 8 / 9, 15 / 16 / 17 and 31 / 32 / 33 the chunk boundaries' two
        # sides that differ -- a list ending on the boundary and the one past it; 8 is the LDS variant's batch)
        for K in (0, 1, 8, 9, 16, 17, 32, 33, 60):
            cases.append(term_case(mp, _spread(K, 0, 60, 7), "spread"))
        return cases
    if mp.kind == "mw":
        U = mp.units
        plans = {2: [(w, M - w), (0, 17), (16, 0)], 3: [(16, 0, 16), (0, 0, 17), (w, w, M - 2 * w)],
                 4: [(15, 1, 0, 33), (0, 0, 0, 17), (16, 0, 16, 0), (w, w, w, M - 3 * w)]}[U]
        for plan in plans[:1] if mp.light else plans:
            plan = [min(c, min(w, M - u * w)) for u, c in enumerate(plan)]
            h = [i for u, c in enumerate(plan) for i in _spread(c, u * w, min(w, M - u * w), 1 if c == min(w, M - u * w) else next(
                s for s in (7, 5, 3, 1) if np.gcd(s, min(w, M - u * w)) == 1))]
            cases.append(term_case(mp, h, "per wave " + "+".join(map(str, plan))))
        return cases
    if mp.kind == "grp" or w < 64:
        for K in (0, 1, w, w + 1, 2 * w):
            cases.append(term_case(mp, _spread(K, 0, M, 1 if K == M else 7), "spread"))
        cases.append(ragged_case(mp))
        return cases
    # k_rollout_w64 with 2 .. 4 slots (and the generic kernel at 64 lanes)
    # (K thinned for the CPU cost of the reference: a list ending on the wave's last chunk boundary and the one past it,
    # top down and alternating; every obstacle a holder at M = 128 and 200)
    for K in {70: (16, 64, 65), 128: (64, 65, 128), 200: (65, 200), 256: (64, 65)}[M]:
        if K == M:
            cases.append(term_case(mp, range(M), "all"))
            continue
        cases.append(term_case(mp, range(M - K, M), "top down"))                       # the highest slot(s)
        if K == 65:
            alt = [(j % 64) + 64 * ((j + j // 64) % mp.units) for j in range(K)]       # alternating slots, lane by lane
            alt = sorted(set(i for i in alt if i < M))
            alt += [i for i in range(M) if i not in alt][:K - len(alt)]
            cases.append(term_case(mp, alt, "alternating slots"))
    return cases


def cases(mp, families=None):
    families = mp.families if families is None else families
    out = []
    if "A" in families:
        out += family_a(mp)
    if "B" in families:
        out += family_b(mp)
    if "C" in families:
        out += family_c(mp)
    # The reference costs about 1 ms per obstacle, agent and step, and a latch of an Obstacle / GoalObstacle agent M
    # norms more. All agents run; shadowed are
    #   family A: every agent up to 64 obstacles, above that one per case, the six types rotating over the cases;
    #   family B: one agent of each type up to 64 obstacles (agents 3 .. 5 repeat the types of 0 .. 2); above that one latch
    #             agent per case, Obstacle and GoalObstacle alternating so that every tie set sees one at rest and the other
    #             moving, and the Goal control in the first case of each variant;
    #   family C: every agent up to 32 obstacles, two to 64, above that one of Had, Goal, Vel, Random (the list does not
    #             depend on the heuristic, and the latches are family B's), rotating; the ragged case all of them
    nb = {False: 0, True: 0}
    for k, c in enumerate(out):
        n = int(c.scene["n_agents"])
        if getattr(c, "all_agents", False):
            continue
        if c.family == "B":
            mv = bool(c.info["moving"])
            c.agents = [0, 1, 2] if mp.M <= 64 else [(nb[mv] + mv) % 2] + ([2] if nb[mv] == 0 else [])
            nb[mv] += 1
        elif mp.M > 64:
            c.agents = [k % n] if c.family == "A" else [(0, 1, 4, 5)[k % 4] % n]
        elif mp.M > 32 and c.family == "C":
            c.agents = sorted({k % n, (k + 3) % n})
    return out


def assert_decided(st, n_cases, n_agents):
    """every agent of every case compared, none undecidable"""
    st.assert_ok(0.0, min_compared=n_cases * n_agents)
    assert st.undecidable == 0, st.report()
