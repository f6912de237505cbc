"""The CPU oracle (oracle/pmaf_oracle.c) against the independent high-precision reference (tests/hp_reference.py).

The parity suite holds the kernels to the oracle bit for bit; that cannot catch a mistake both make. Here the oracle
is shadowed, one tick or one stepping call at a time on its own fp64 state, by a restatement that shares no code and no
evaluation order with it and carries a rounding-error bound (tests/hp_shadow.py). Also: self-tests of the bound, the
exact-tie scenes (tests/hp_edges.py) and the module's independence. Run with -s to see the per-case report.
"""
import ast
import os

import numpy as np
import pytest

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
