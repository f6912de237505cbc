"""Scenes whose number K of terms in the ordered force sum (circ_and_scale_w64's `count`) VARIES along one rollout, for
the two step loops of the one-slot DPP sum (csrc/pmaf_rollout_w64_body.hpp): a wave runs the short loop until its first
step with K > 16 and the long loop, which adds the list's second chunk whatever K is, from the next step to the end of
the rollout. tests/test_long_loop.py checks on the CPU oracle that the K sequences named below really occur,
tests/test_long_loop_gpu.py runs the cases on the kernels.

How K is steered. The agents fly along the x axis at vel_max = 2 m/s with dt = 0.2 s: 0.4 m per step. The manager's
initial position IS the start and no obstacle is within the shell there, so the real agent's first step is the
attractor's alone (gain x dt = 1) and takes it to START + 0.2 m at vel_max; every later step of the real agent and of the rollouts starts on-speed,
where the attractor's velocity error is zero, and advances 0.4 m. So the rollout of tick t visits, at its step k, the
lattice point x_j = START.x + 0.2 + 0.4 j with j = t + k, up to the small deflection by the circular forces (k_circ is
small; tests/test_long_loop.py measures what the margins leave of it).

The field obstacles come in CLUSTERS, rings round the axis: all obstacles of a cluster share the axial position xc and
the distance rho from the axis. A cluster gives terms while it is ahead (behind the agent it is skipped, :84-88) and
inside the detect shell, that is at the lattice points j with s <= j < e (s >= 1: nothing at the start itself): xc lies half a step behind x_e (0.2 m from
either neighbouring lattice point) and rho is chosen so that the shell is crossed half a step in front of x_s. With a
shell of 2 m and windows of 2 ... 4 steps every obstacle is then at least 0.14 m from the shell surface at every
lattice point (the issue asks for 0.05 m). A MOVING cluster flies head-on at -vel_max: it closes 0.8 m per step, the
list is handed to every tick unadvanced, and every distance stays on the half-step lattice at every tick.

Imports neither oracle/ nor the package: planners are handed in."""
import numpy as np

M, N_AGENTS = 60, 7
H = 0.4                 # metres per step at vel_max
DT, VMAX = 0.2, 2.0
SHELL, RAD, ORAD = 2.0, 0.05, 0.03
REACH = SHELL + RAD + ORAD          # centre distance at which an obstacle's surface touches the shell
MARGIN = 0.05
START = np.array([-8.0, 0.0, 0.7])
GOAL = START + np.array([40.0, 0.0, 0.0])
INIT = START.copy()
SENT_RADIUS = 0.1


def lattice(j):
    """x of lattice point j (the start of step k of tick t, j = t + k)"""
    return START[0] + 0.5 * H + H * j


# (obstacles, first lattice index, one past the last) per cluster
SCENES = {
    # nothing -> short (3) -> long (25) -> short (3: the stale second chunk) -> nothing in the shell -> long again (26),
    # which is the last step of ticks 0 and 1 at capacity 11 (lattice points 9 and 10)
    "runs": dict(cap=11, clusters=[(3, 1, 3), (25, 3, 5), (3, 5, 7), (26, 8, 11)]),
    # long (17; the FIRST step of ticks 1 and 2), then inside the long loop 16, 17, 33, 32, 16, 16, nothing
    "bounds": dict(cap=10, clusters=[(17, 1, 3), (16, 3, 7), (1, 4, 6), (16, 5, 9)]),
}


def k_at(name, j, moving=False, tick=0):
    """K at lattice point j (step j - tick of tick `tick`: the head-on cluster's place depends on both)"""
    if moving != "cluster":
        return sum(n for n, s, e in SCENES[name]["clusters"] if s <= j < e)
    k = j - tick
    tot = sum(n for n, s, e in SCENES[name]["clusters"][:-1] if s <= j < e)
    n, s, e = SCENES[name]["clusters"][-1]
    return tot + (n if 0.0 < _moving_rel(s, e, tick, k) < H * _moving_window(s, e) else 0)


def _moving_window(s, e):
    return 4           # the head-on cluster's shell window in static steps (1.6 m): two of its 0.8 m steps


def _moving_rel(s, e, tick, k):
    """axial distance from the agent to the head-on cluster at step k of tick `tick`: in tick 0 it is passed between
    steps e - 2 and e - 1 (the capacity's last step is e - 2, a long one)"""
    c0 = 0.5 * H + 2.0 * H * (e - 2)
    return c0 - H * tick - 2.0 * H * k


def build_scene(scenes, name, moving=False, sent_near=False, n_agents=N_AGENTS):
    """scenes: the package's scenes module. moving (the bodies that advance the obstacles): "cluster" -- the last cluster
    flies head-on; "far" -- a far obstacle moves away and K is what it is at rest. sent_near: the repulsive obstacle
    stands 0.6 m beside the third lattice point, in repelForce's range for most of the rollout, instead of 170 m away.
    n_agents: a larger population (more waves than SIMDs) -- the seven types repeated, the random vectors drawn in the
    same order, so agents 0 ... 6 are the default call's agents (tests/test_variant_matrix.py asserts it)."""
    spec = SCENES[name]
    rng = np.random.default_rng(5200 + sorted(SCENES).index(name))
    rows = []
    for ci, (n, s, e) in enumerate(spec["clusters"]):
        mv = moving == "cluster" and ci == len(spec["clusters"]) - 1
        if mv:
            w = H * _moving_window(s, e)
            xc = lattice(0) + _moving_rel(s, e, 0, 0)
        else:
            w = H * (e - s)
            xc = lattice(e) - 0.5 * H
        assert w < REACH - 0.1
        rho = np.sqrt(REACH * REACH - w * w)
        ang = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
        for a in ang:
            rows.append([xc, START[1] + rho * np.cos(a), START[2] + rho * np.sin(a), -VMAX if mv else 0.0, 0.0, 0.0, ORAD])
    assert len(rows) <= M
    while len(rows) < M:        # the other lanes: far off, never in the shell
        rows.append([START[0] + rng.uniform(0.0, 10.0), 60.0 + 2.0 * len(rows), START[2], 0.0, 0.0, 0.0, ORAD])
    if moving == "far":
        rows[-1][3:6] = [0.0, 0.5, 0.0]
    else:
        assert moving in (False, "cluster")
    rows = [rows[i] for i in rng.permutation(M)]       # the clusters' members spread over the lanes
    if sent_near:
        rows.append([lattice(2), 0.6, START[2], 0.0, 0.0, 0.0, SENT_RADIUS])
    else:
        rows.append([100.0, 100.0, 100.0, 0.0, 0.0, 0.0, SENT_RADIUS])
    obs = np.asarray(rows, dtype=np.float64)
    assert n_agents >= N_AGENTS
    rv = rng.uniform(-1.0, 1.0, (n_agents, M + 1, 3))
    rv /= np.linalg.norm(rv, axis=-1, keepdims=True)
    types = np.resize(scenes.default_agent_types(N_AGENTS), n_agents)
    return dict(name="long_loop_%s%s%s" % (name, ("_" + moving) if moving else "", "_sent" if sent_near else ""),
                n_agents=n_agents, max_prediction_steps=spec["cap"], dt=DT, velocity_max=VMAX, approach_dist=0.25,
                detect_shell_rad=SHELL, agent_mass=1.0, radius=RAD, k_attr=5.0, k_circ=0.01, k_repel=0.002, k_damp=5.0,
                cost_gains=np.array([100.0, 10.0, 0.001, 1.0]), ws_limits=np.array([40.0, -10.0, 3.0, -3.0, 3.0, -2.0]),
                start=START.copy(), goal=GOAL.copy(), obstacles=obs, random_vecs=rv,
                agent_types=types)    # Had, Goal, Obstacle, GoalObstacle, Vel, Random x 2 (repeated)


def cases():
    """(scene, moving, sent_near) of the plain handles"""
    return [("runs", False, False), ("runs", "cluster", False), ("runs", False, True), ("runs", "cluster", True),
            ("bounds", False, False), ("bounds", "far", False), ("bounds", False, True)]


def prepare(planner):
    """put a fresh planner (created with mgr_init_pos = INIT) at the start of the first tick"""
    planner.set_real_position(START)
