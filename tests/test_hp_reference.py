"""The CPU oracle (oracle/pmaf_oracle.c) against the independent high-precision reference (tests/hp_reference.py).

The parity suite holds the kernels to the oracle bit for bit; that cannot catch a mistake both make. Here the oracle
is shadowed, one tick or one stepping call at a time on its own fp64 state, by a restatement that shares no code and no
evaluation order with it and carries a rounding-error bound (tests/hp_shadow.py). Also: self-tests of the bound, the
exact-tie scenes (tests/hp_edges.py) and the module's independence. Run with -s to see the per-case report.
"""
import ast
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as graft
import hp_anchored as ha
import hp_edges
import hp_reference as hp
import hp_shadow as sh

HERE = os.path.dirname(os.path.abspath(__file__))

_CASES = {}


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


def _run_case(name, orc, scenes):
    """each case runs once per session; the branch-coverage test reads every case's table"""
    if name not in _CASES:
        _CASES[name] = CASES[name](orc, scenes)
    return _CASES[name]


def _ticks(orc, scenes, scene, n_ticks, name, dynamic=False, agents=None, policy="xact", switch=False):
    A = hp.Arith(policy)
    st = sh.Stats(name)
    pl = orc.OraclePlanner(scene, mgr_init_pos=scene["start"])
    # init_pos 0.25 m from the real agent: the step's gate is open from the first tick
    ip = sh.start(pl, scene, init_pos=scene["start"] + np.array([0.0, 0.0, -0.25]), real_pos=scene["start"])
    obs = scene["obstacles"].copy()
    for t in range(n_ticks):
        if switch and t:
            # install the agent whose rollout ended farthest from the goal as best_agent_: the hysteresis switches
            paths, n = pl.paths()
            far = int(np.argmax(np.linalg.norm(paths[np.arange(len(n)), n - 1] - scene["goal"], axis=1)))
            pl.set_best(far + 1, sh.agent_types(scene)[far], scene["random_vecs"][far])
        sh.shadow_tick(pl, scene, obs, ip, A, st, agents=agents)
        if dynamic:
            obs = scenes.advance_live_obstacles(obs)
    pl.close()
    return st


def case_c1_one_step(orc, scenes):
    return _ticks(orc, scenes, scenes.static1_scene(16, 1), 40, "C1 one-step")


def case_dyn1_one_step(orc, scenes):
    # 10 agents: all six heuristics (Had, Goal, Obstacle, GoalObstacle, Vel, Random x5), moving spheres
    return _ticks(orc, scenes, scenes.dyn1_scene(10, 1), 40, "dyn1 one-step", dynamic=True)


def case_c1_k_step(orc, scenes):
    return _ticks(orc, scenes, scenes.static1_scene(16, 20), 3, "C1 20-step", switch=True)


def case_c2r_k_step(orc, scenes):
    # C2 reduced: 8 agents, 16 moving spheres, 12-step horizon
    sc = scenes.synthetic_scene(8, 12, 16, config_id=2, dynamic=True)
    return _ticks(orc, scenes, sc, 4, "C2r 12-step dyn", dynamic=True)


def case_stepping(orc, scenes):
    A = hp.Arith("xact")
    st = sh.Stats("stepping API")
    sc = scenes.synthetic_scene(8, 40, 16, config_id=2, dynamic=True)
    pl = orc.OraclePlanner(sc, mgr_init_pos=sc["start"])
    ip = sh.start(pl, sc)
    # mid-way, moving at 0.15 m/s: the gate is open and several spheres are inside the shell
    pl.set_agent_pos_and_vels(np.array([-0.2, 0.05, 0.68]), np.array([0.15, -0.01, 0.02]))
    sh.shadow_steps(pl, sc, sc["obstacles"], ip, A, st, 25)
    pl.close()
    return st


def case_link_force(orc, scenes):
    A = hp.Arith("xact")
    st = sh.Stats("link_force / eval_obstacle_distance")
    sc = scenes.static1_scene(16, 4)
    obs = sc["obstacles"].copy()
    obs[-1, :3] = [0.1, 0.05, 0.8]               # the repulsive obstacle among the links
    rng = np.random.default_rng(5)
    lp = obs[-1, :3] + rng.uniform(-0.4, 0.4, (48, 3))
    lp[0] = obs[-1, :3]                           # centre on the obstacle: zero direction, floored distance
    lp[1] = obs[-1, :3] + [0.0, 0.0, 0.5]         # |p - o| - (0.05 + 0.1) = 0.35 = shell: out (exact tie)
    lp[2] = obs[-1, :3] + [0.0, 0.0, 0.15]        # touching: distance 0 -> floor
    kr = rng.uniform(0.01, 0.1, 48)
    pl = orc.OraclePlanner(sc, mgr_init_pos=sc["start"])
    sh.start(pl, sc)
    sh.shadow_link_force(pl, sc, lp, kr, obs, A, st)
    for p in lp[::6]:
        pl.set_agent_positions(p)
        sh.shadow_eval_obstacle_distance(pl, sc, obs, A, st)
    pl.close()
    return st


def case_edges(orc, scenes):
    st = sh.Stats("exact-tie scenes")
    A = hp.Arith("xact")
    for edge in hp_edges.EDGES:
        edge.run(lambda sc: orc.OraclePlanner(sc, mgr_init_pos=sc["start"]), A, st)
    return st


CASES = {
    "c1_one_step": case_c1_one_step,
    "dyn1_one_step": case_dyn1_one_step,
    "c1_k_step": case_c1_k_step,
    "c2r_k_step": case_c2r_k_step,
    "stepping": case_stepping,
    "link_force": case_link_force,
    "edges": case_edges,
}


# K-step rollouts: the bound of a step is driven by k_circ / d^2 and its derivative, and near a sphere (d ~ 1 cm) it grows
# several-fold per step, as a worst-case fp64 error can; rollouts whose branches it stops deciding are not compared
MAX_UNDECIDABLE = {"c1_k_step": 0.10, "c2r_k_step": 0.10}


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_within_reference_bound(orc, scenes, name):
    """every oracle output within the reference's rounding-error bound, every decided branch on the same side"""
    st = _run_case(name, orc, scenes)
    st.assert_ok(max_undecidable=MAX_UNDECIDABLE.get(name, 0.02))


def test_edge_scenes_decide_their_ties(orc, scenes):
    """each exact-tie scene is decided by the reference with bound 0 at its tie (not skipped as undecidable)"""
    st = _run_case("edges", orc, scenes)
    assert st.undecidable == 0, st.report()
    for edge in hp_edges.EDGES:
        assert edge.tie_seen, "%s: the tie was never evaluated" % edge.name


def test_branch_coverage(orc, scenes):
    """over all cases, both outcomes of every branch of the step, the guard, the evaluation and the stepping API were
    seen among decided samples"""
    seen = {}
    for name in CASES:
        for k, v in _run_case(name, orc, scenes).seen.items():
            seen.setdefault(k, set()).update(v)
    missing = [b for b in hp.BRANCHES if seen.get(b, set()) != {True, False}]
    print("branch coverage:", {b: sorted(seen.get(b, ())) for b in hp.BRANCHES})
    assert not missing, "branches without both outcomes: %s" % missing


# ---------------------------------------------------------------------------------------------------------------------
# self-tests of the bound
# ---------------------------------------------------------------------------------------------------------------------
def _np_dot(a, b, right=False):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]) if right else (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def test_bound_holds_for_fp64_expressions():
    """plain fp64 evaluations (both dot associations) of random dots, norms, normalisations, cross products and
    quotients lie within the carried bound, and the bound is not uselessly loose: some shaped case reaches > 10 %"""
    A = hp.Arith("xact")
    rng = np.random.default_rng(11)
    worst = 0.0
    for t in range(400):
        s = 10.0 ** rng.uniform(-3, 1)
        a, b = rng.uniform(-s, s, 3), rng.uniform(-1, 1, 3)
        if t % 4 == 0:      # shaped: nearly cancelling dot product
            b = np.array([a[1], -a[0], 0.0]) + rng.uniform(-1e-6, 1e-6, 3)
        qa, qb = A.v3(a), A.v3(b)
        for right in (False, True):
            d = _np_dot(a, b, right)
            n = np.sqrt(_np_dot(a, a, right))
            checks = [(A.dot(qa, qb), d), (A.norm(qa), n)]
            qn = A.normalized(qa)
            checks += [(qn[k], a[k] / n) for k in range(3)]
            cr = A.cross(qa, qb)
            npc = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
            checks += [(cr[k], npc[k]) for k in range(3)]
            checks.append((A.div(A.dot(qa, qb), A.norm(qa)), d / n))
            # a chained expression: the circular term's direction v x (c x v) for v = a / |a|
            cv = A.cross(qn, A.cross(A.normalized(qb), qn))
            bn = b / np.sqrt(_np_dot(b, b, right))
            an = a / n
            inner = np.array([bn[1] * an[2] - bn[2] * an[1], bn[2] * an[0] - bn[0] * an[2], bn[0] * an[1] - bn[1] * an[0]])
            outer = np.array([an[1] * inner[2] - an[2] * inner[1], an[2] * inner[0] - an[0] * inner[2],
                              an[0] * inner[1] - an[1] * inner[0]])
            checks += [(cv[k], outer[k]) for k in range(3)]
            for q, x in checks:
                r = hp.excess(q, x)
                assert r <= 1.0, (t, right, q, x, r)
                worst = max(worst, r)
    print("worst fp64 error / bound: %.3f" % worst)
    assert worst > 0.1


def test_exact_operations_carry_no_bound():
    """exact doubles in, an exactly representable result out: bound 0 under the strict policies (the tie scenes rest
    on this), a non-zero bound where the result rounds or the policy's / and sqrt are not correctly rounded"""
    A = hp.Arith("xact")
    v = A.v3((0.375, 0.5, 0.0))
    n = A.norm(v)
    assert n.v == hp.MPF(0.625) and n.e == 0.0
    assert A.norm(A.v3((0.1, 0.0, 0.0))).e == 0.0          # sqrt(fl(x * x)) = |x|
    assert A.div(A.c(1.0), A.c(3.0)).e > 0.0
    assert A.add(A.c(0.1), A.c(0.2)).e > 0.0
    F = hp.Arith("fast")
    assert F.norm(F.v3((0.375, 0.5, 0.0))).e > 0.0
    assert F.mul(F.c(0.5), F.c(3.0)).e == 0.0
    with pytest.raises(hp.Undecidable):
        A.decide("x", A.add(A.c(0.1), A.c(0.2)), "<", A.c(0.30000000000000004))
    assert A.decide("x", A.c(13.0), ">", A.c(13.0)) is False


# ---------------------------------------------------------------------------------------------------------------------
# independence
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_is_independent_of_the_oracle_and_the_package():
    """hp_reference.py imports neither oracle/ (orc.py, the C oracle) nor the package or its ctypes layer"""
    src = open(os.path.join(HERE, "hp_reference.py")).read()
    tree = ast.parse(src)
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add(node.module or "")
        elif isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", "")) in ("__import__", "import_module"):
            raise AssertionError("dynamic import in hp_reference.py")
    assert mods <= {"math", "itertools", "mpmath.ctx_mp"}, mods
    for bad in ("oracle", "orc", "ctypes", "pmaf", "torch", "numpy"):
        assert not any(m == bad or m.startswith(bad + ".") for m in mods), bad


# ---------------------------------------------------------------------------------------------------------------------
# anchored walks: every step of full-length rollouts (tests/hp_anchored.py)
# ---------------------------------------------------------------------------------------------------------------------
ANCHORED_MAX_UNDECIDABLE = 0.02


def _task_scene(scenes, name):
    recs = json.load(open(os.path.join(HERE, "golden", "task_scenes.json")))
    return scenes.scene_from_record(recs[name], name)


def _anchored_ticks(orc, scenes, scene, n_ticks, name, agents, frac, dynamic=False, walk_from=0, policy="xact",
                    eval_agents=None):
    """n_ticks planCallback ticks of the oracle; from tick walk_from on every sampled agent's rollout is walked"""
    A = hp.Arith(policy)
    st = sh.Stats(name)
    st.evaluation = sh.Stats(name + ", every cost and the selection")    # (its own counts: st's cap is unchanged)
    pl = orc.OraclePlanner(scene, mgr_init_pos=scene["start"])
    try:
        ip = sh.start(pl, scene, init_pos=scene["start"] + np.array([0.0, 0.0, -0.25]), real_pos=scene["start"])
        obs = scene["obstacles"].copy()
        for t in range(n_ticks):
            sh.shadow_tick(pl, scene, obs, ip, A, st, agents=agents if t >= walk_from else [],
                           rollouts=ha.walker(frac, seed=t), eval_agents=eval_agents, eval_stats=st.evaluation)
            if dynamic:
                obs = scenes.advance_live_obstacles(obs)
    finally:
        pl.close()
    return st


class PopOracles:
    """P oracle planners presented as one P-population planner (the [P, ...] getters of PmafPlanner). coupling
    {p: (src_pop, radius)} replaces population p's trailing obstacle by population src_pop's previous real position,
    velocity 0 (include/pmaf.h "peer mailboxes"), as the device-side coupling does"""

    def __init__(self, orc, scs, coupling=None):
        self.P = len(scs)
        self.pl = [orc.OraclePlanner(s, mgr_init_pos=s["start"]) for s in scs]
        self.coupling = coupling or {}

    def close(self):
        for q in self.pl:
            q.close()

    def _each(self, name, *args):
        return [getattr(q, name)(*args) for q in self.pl]

    def set_initial_position(self, pos):
        for q, x in zip(self.pl, np.reshape(pos, (self.P, 3))):
            q.set_initial_position(x)

    def set_real_position(self, pos):
        for q, x in zip(self.pl, np.reshape(pos, (self.P, 3))):
            q.set_real_position(x)

    def tick(self, obstacles, dt, cost_gains, ws):
        obs = np.array(obstacles, dtype=np.float64).reshape(self.P, -1, 7)
        prev = [q.real_state()[0] for q in self.pl]
        for p, (src, radius) in self.coupling.items():
            obs[p, -1] = list(prev[src]) + [0.0, 0.0, 0.0, radius]
        return np.array([q.tick(obs[p], dt, cost_gains, ws) for p, q in enumerate(self.pl)])

    def real_state(self):
        return [np.stack(x) for x in zip(*self._each("real_state"))]

    def real_known(self):
        return [np.stack(x) for x in zip(*self._each("real_known"))]

    def paths(self):
        return [np.stack(x) for x in zip(*self._each("paths"))]

    def best(self):
        return np.array(self._each("best_type")), np.array(self._each("best_id"))


for _m in ("agent_vel", "min_obs_dist", "rot_vecs", "known", "success", "costs"):
    setattr(PopOracles, _m, (lambda m: lambda self: np.stack(self._each(m)))(_m))


def _pop_case(orc, scenes, name, coupling=None, swap_goals=False, n_ticks=3):
    """C4-shaped: two arms, each arm's trailing obstacle the other arm's end effector. coupling None: coupled on the
    host (shard.DualArmCoupling builds the rows the planner and the shadow both get); otherwise coupled inside the
    planner and rebuilt by the shadow (hp_shadow.coupled_rows)"""
    arms = scenes.dual_arm_scenes(16, 150, 12)
    starts = np.stack([s["start"] for s in arms])
    made = [dict(s) for s in arms]
    if swap_goals:                                   # a planner that mixes up the per-population goal
        made[0]["goal"], made[1]["goal"] = arms[1]["goal"], arms[0]["goal"]
    A = hp.Arith("xact")
    st = sh.Stats(name)
    pl = PopOracles(orc, made, coupling)
    try:
        pl.set_initial_position(starts)
        obs = np.stack([s["obstacles"] for s in arms])
        host = None if coupling else graft.load_package().shard.DualArmCoupling(obs, 0.1)
        for t in range(n_ticks):
            rows = host.coupled_obstacles(pl.real_state()[0]) if host else obs
            sh.shadow_tick(pl, arms, rows, starts, A, st, agents=[0, 5], rollouts=ha.walker(0.5, seed=t),
                           coupling=coupling)
    finally:
        pl.close()
    return st


def case_anchored_c2(orc, scenes):
    # (one tick: the scored paths are the one-point initial ones, every cost ties and index 0 must win -- all 64 compared)
    return _anchored_ticks(orc, scenes, scenes.config_scene("C2"), 1, "anchored C2", list(range(0, 64, 8)), 0.5,
                           eval_agents="all")


def case_anchored_c5_scene1(orc, scenes):
    sc = scenes.config_scene("C5", scene_id=1, dynamic=True)
    return _anchored_ticks(orc, scenes, sc, 3, "anchored C5 scene 1 dyn", [3, 7, 500, 1001], 0.25, dynamic=True)


def case_anchored_c3(orc, scenes):
    return _anchored_ticks(orc, scenes, scenes.config_scene("C3"), 1, "anchored C3", [17], 0.1)


def case_anchored_kobo1(orc, scenes):
    sc = _task_scene(scenes, "sim_kobo_dyn_spheres1")
    return _anchored_ticks(orc, scenes, sc, 2, "anchored sim_kobo_dyn_spheres1", [4], 0.1, dynamic=True, walk_from=1)


def case_anchored_pop_host(orc, scenes):
    return _pop_case(orc, scenes, "anchored C4-shaped, P = 2, coupled on the host")


def case_anchored_pop_mailbox(orc, scenes):
    return _pop_case(orc, scenes, "anchored C4-shaped, P = 2, coupled in the planner", coupling={0: (1, 0.1), 1: (0, 0.1)})


ANCHORED = {
    "anchored_c2": case_anchored_c2,
    "anchored_c5_scene1": case_anchored_c5_scene1,
    "anchored_c3": case_anchored_c3,
    "anchored_kobo1": case_anchored_kobo1,
    "anchored_pop_host": case_anchored_pop_host,
    "anchored_pop_mailbox": case_anchored_pop_mailbox,
}
CASES.update(ANCHORED)


@pytest.mark.parametrize("name", list(ANCHORED))
def test_oracle_anchored_rollouts(orc, scenes, name):
    """every step of full-length rollouts (200-1500 steps) within the reference's bound from the oracle's own state at
    that step; the guard, success, min_obs_dist, known flags, latched rotation vectors and final velocity"""
    st = _run_case(name, orc, scenes)
    assert st.walk.horizon >= 150, st.report()
    st.assert_ok(max_undecidable=ANCHORED_MAX_UNDECIDABLE, min_compared=10)
    if name == "anchored_c2":
        st.evaluation.assert_ok(0.0, min_compared=65)
        assert st.evaluation.selections == 1, st.evaluation.report()


# -- teeth: planners that are wrong in small ways must fail -----------------------------------------------------------
def _tick_then(orc, scene, n_ticks, dynamic, scenes):
    """an oracle after n_ticks ticks, with its rollout's inputs and outputs"""
    pl = orc.OraclePlanner(scene, mgr_init_pos=scene["start"])
    ip = sh.start(pl, scene, init_pos=scene["start"] + np.array([0.0, 0.0, -0.25]), real_pos=scene["start"])
    obs = scene["obstacles"].copy()
    for t in range(n_ticks):
        pre = sh.snapshot(pl)
        pl.tick(obs, scene["dt"], scene["cost_gains"], scene["ws_limits"])
        rows = obs
        if dynamic:
            obs = scenes.advance_live_obstacles(obs)
    return pl, ip, pre, sh.snapshot(pl), rows


def _walk(scene, ip, pre, post, rows, i, frac=1.0, policy="xact"):
    A = hp.Arith(policy)
    st = sh.Stats("mutant")
    ha.walk_agent(A, st, scene, i, post["real_pos"], post["real_vel"], post["real_known"], pre["rot_vecs"][i],
                  pre["success"], post, rows, ip, frac=frac)
    print(st.report())
    return st


def _fails_with(st, what):
    assert st.failures, "the mutant passed:\n" + st.report()
    assert any(what in f for f in st.failures), "failed, but not for %r: %s" % (what, st.failures[:4])


@pytest.fixture(scope="module")
def c2_tick(orc, scenes):
    sc = scenes.config_scene("C2")
    pl, ip, pre, post, rows = _tick_then(orc, sc, 1, False, scenes)
    pl.close()
    return sc, ip, pre, post, rows


def test_mutant_interior_point_256_ulp(orc, scenes):
    """one interior path point (step 150) moved by 256 ulp. The walk's resolution there is set by the velocity ball: after
    150 steps its radius (the sum of every step's position rounding, 2 |dp| / dt each) is ~6e-12 m/s, and even the
    second-difference check, from which the radius drops out, carries the force's sensitivity to it -- ~1e-14 m, about
    100 ulp, on this free-space stretch of sim_kobo_dyn_spheres1 (~1e-13 m near C2's spheres). 64 ulp is below that."""
    sc = _task_scene(scenes, "sim_kobo_dyn_spheres1")
    sc["max_prediction_steps"] = 201
    pl, ip, pre, post, rows = _tick_then(orc, sc, 1, True, scenes)
    pl.close()
    i = 3
    assert post["n"][i] > 180
    ok = _walk(sc, ip, pre, post, rows, i)
    assert not ok.failures and ok.undecidable == 0, ok.report()
    post = dict(post, paths=post["paths"].copy())
    c = int(np.argmax(np.abs(post["paths"][i, 150])))
    x = post["paths"][i, 150, c]
    post["paths"][i, 150, c] = x + 256 * np.spacing(x)
    _fails_with(_walk(sc, ip, pre, post, rows, i), "path[150]")


def test_mutant_last_steps_longer_dt(c2_tick):
    """a path whose last 10 steps were integrated with dt (1 + 1e-9): each of their increments scaled by 1 + 1e-9"""
    sc, ip, pre, post, rows = c2_tick
    i = 16
    n = int(post["n"][i])
    post = dict(post, paths=post["paths"].copy())
    p = post["paths"][i]
    orig = p[:n].copy()
    for k in range(n - 10, n):
        p[k] = p[k - 1] + (orig[k] - orig[k - 1]) * (1.0 + 1e-9)
    _fails_with(_walk(sc, ip, pre, post, rows, i, frac=0.0), "path[%d]" % (n - 1))


@pytest.fixture(scope="module")
def c5_tick(orc, scenes):
    sc = scenes.config_scene("C5", scene_id=1, dynamic=True)
    pl, ip, pre, post, rows = _tick_then(orc, sc, 3, True, scenes)
    return sc, pl, ip, pre, post, rows


def test_mutant_obstacles_advanced_before_the_step(orc, c5_tick):
    """the rollout's private obstacles predicted BEFORE each step instead of after: the same oracle, reset with rows
    advanced by one predictObstacles"""
    sc, pl, ip, pre, post, rows = c5_tick
    i = 7
    adv = rows.copy()
    adv[:, 0:3] = adv[:, 0:3] + sc["dt"] * adv[:, 3:6]
    pl.reset_agents(post["real_pos"], post["real_vel"], adv)
    pl.rollout()
    bad = sh.snapshot(pl)
    _fails_with(_walk(sc, ip, pre, bad, rows, i, frac=0.1), "path[")


def test_mutant_latch_one_step_late(c5_tick):
    """a latch one step late: the latched rotation vector the planner reports is the one of the next path point"""
    sc, pl, ip, pre, post, rows = c5_tick
    for i in (3, 7, 500):
        st = _walk(sc, ip, pre, post, rows, i, frac=0.0)
        assert not st.failures, st.report()
        if st.walk.latches:
            break
    _, k, j = st.walk.latches[0]
    A = hp.Arith("xact")
    own = hp.obstacles_from_rows(A, rows, radii=sc["obstacles"][:, 6])
    for _ in range(k + 1):
        hp.predict_obstacles(A, own, sc["dt"])
    late = hp.rotation_vector(A, sh.agent_types(sc)[i], A.v3(post["paths"][i, k + 1]), A.v3(sc["goal"]), own, j,
                              [A.v3(r) for r in sc["random_vecs"][i]])
    bad = dict(post, rot_vecs=post["rot_vecs"].copy())
    bad["rot_vecs"][i, j] = [q.f for q in late]
    _fails_with(_walk(sc, ip, pre, bad, rows, i, frac=0.0), "rot[%d] latched at step %d" % (j, k))


def test_mutant_population_goals_swapped(orc, scenes):
    """a two-population planner that gives each population the other's goal"""
    st = _pop_case(orc, scenes, "mutant: goals swapped", swap_goals=True, n_ticks=1)
    print(st.report())
    assert st.failures, st.report()
    assert any("path[" in f or "real pos" in f for f in st.failures), st.failures[:4]


# -- the ball itself ---------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _update(p, v, a, dt, vmax, form):
    """updatePositionAndVelocity in fp64, one of the operation sequences the policies may use"""
    half = ((0.5 * a) * dt) * dt
    if form == "left":
        p1 = (p + half) + v * dt
    elif form == "right":
        p1 = p + (half + v * dt)
    else:                                        # fma(dt, v, p) + half, and fma(dt, a, v)
        p1 = np.array([_fma(dt, v[k], p[k]) for k in range(3)]) + half
    u = np.array([_fma(dt, a[k], v[k]) for k in range(3)]) if form == "fma" else v + a * dt
    un = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    if un > vmax:
        u = u * (vmax / un)
    return p1, u


@pytest.mark.parametrize("policy,form", [("xact", "left"), ("xact", "right"), ("fma", "fma"), ("fast", "left")])
def test_ball_contains_fp64_velocity(policy, form):
    """for random positions, velocities in a ball, accelerations |a| <= 13 and both clamp outcomes, the ball that
    hp_anchored derives from the two fp64 positions contains the fp64 velocity, under the operation sequence given"""
    A = hp.Arith(policy)
    rng = np.random.default_rng(23)
    worst, n, clamped = 0.0, 0, set()
    for t in range(300):
        dt = [0.01, 0.02, 0.0625][t % 3]
        vmax = rng.uniform(0.1, 0.6)
        p = rng.uniform(-1.0, 1.0, 3)
        c = rng.normal(size=3)
        c *= vmax * rng.uniform(0.3, 1.0) / np.linalg.norm(c)
        r = [0.0, 1e-13, 1e-11][t % 3]
        d = rng.normal(size=3)
        v = c + d * (r * rng.uniform(0, 1) / np.linalg.norm(d))
        a = rng.normal(size=3)
        a *= rng.uniform(0, 13.0) / np.linalg.norm(a)
        if t % 5 == 0:
            a *= 13.0 / np.linalg.norm(a)
        p1, v1 = _update(p, v, a, dt, vmax, form)
        ball = ha.Ball([hp.MPF(float(x)) for x in c], r)
        try:
            nb = ball.advance(A, p, p1, dt, vmax)
        except hp.Undecidable:
            continue
        clamped.update(A.seen.get("vel_clamp", ()))
        q = nb.ratio(v1)
        assert q <= 1.0, (t, q, nb.r)
        worst, n = max(worst, q), n + 1
    print("%s / %s: %d samples, worst |v - c| / r = %.3g" % (policy, form, n, worst))
    assert n >= 250 and clamped == {True, False}


def test_new_shadow_modules_are_independent_of_the_oracle_and_the_package():
    """hp_anchored.py, hp_shadow.py, hp_select.py and hp_layout.py read planners only through the object handed to them: no
    import of oracle/, the package, ctypes or torch"""
    for name in ("hp_anchored.py", "hp_shadow.py", "hp_select.py", "hp_layout.py"):
        tree = ast.parse(open(os.path.join(HERE, name)).read())
        mods = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                mods.update(a.name for a in node.names)
            elif isinstance(node, ast.ImportFrom):
                mods.add(node.module or "")
            elif isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", "")) in ("__import__", "import_module"):
                raise AssertionError("dynamic import in %s" % name)
        assert mods <= {"math", "numpy", "hp_reference", "hp_shadow"}, (name, mods)
