"""Scenes with a chosen number K of terms in the ordered force sum (circ_and_scale_w64's `count`) at the first step of
every rollout: the one-slot DPP sum of csrc/pmaf_rollout_w64.hpp adds its list in chunks of 16 entries, the first chunk
in the block of the attractor-scaling chain, every further one in a loop that prefetches its successor, so K runs over
both sides of every chunk boundary. tests/test_sum_chunks.py checks the construction on the CPU oracle,
tests/test_sum_chunks_gpu.py runs the cases on the kernels.

M = 60 field obstacles (one slot per lane, the DPP sum), capacity 9, seven agents: one of each heuristic and a second
Random. K obstacles lie at least 0.05 m INSIDE the detect shell round the start point, in the hemisphere towards the
goal (never skipped: ron . gn > 0), the other M - K at least 0.05 m OUTSIDE it; the holders' indices are spread over
the lanes. The manager's initial position lies 0.25 m behind the start, so the gate (cf_agent.cpp:315-317) is open
from the first step although the agents start slowly. Over the three ticks of eight steps the agents move less than
0.05 m (vel_max 0.2 m/s, dt 0.01 s), so the margins hold K for every step of every tick.

Imports neither oracle/ nor the package: planners are handed in."""
import numpy as np

M, CAP, N_AGENTS = 60, 9, 7
KS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 60)
TRACK_KS = (17, 33)
MARGIN = 0.05
START = np.array([-0.6, 0.0, 0.7])
GOAL = np.array([0.6, 0.0, 0.7])
INIT = START - np.array([0.25, 0.0, 0.0])       # >= 0.2 m from the start: the gate is open at step 0
ORAD = 0.03
SENT_RADIUS = 0.1
MOVER_VEL = np.array([0.05, 0.02, -0.01])


def _unit_towards_goal(rng):
    """a direction with x >= 0.3: in front of the agent as seen towards the goal"""
    while True:
        u = rng.uniform(-1.0, 1.0, 3)
        n = np.linalg.norm(u)
        if n > 0.1 and u[0] / n >= 0.3:
            return u / n


def holders(K):
    """the K obstacle indices inside the shell: spread over the lanes, not a prefix"""
    return sorted((7 * j + 2) % M for j in range(K))


def build_scene(scenes, K, moving=False, sent_near=False):
    """scenes: the package's scenes module (parameters and agent types). moving: the outermost far obstacle moves (away:
    it stays outside; with K = M, where there is none, a holder in the middle of the shell moves and stays inside) --
    the kernels then take the bodies that advance the obstacles. sent_near: the repulsive
    obstacle sits 0.3 m beside the start, inside repelForce's range, instead of 170 m away."""
    assert 0 <= K <= M
    rng = np.random.default_rng(4100 + K)
    rad, shell = 0.05, 0.35
    inside = set(holders(K))
    rows = []
    far_r = []
    for i in range(M):
        u = _unit_towards_goal(rng)
        if i in inside:
            d = rng.uniform(0.06, shell - MARGIN - 0.01)            # surface distance, >= MARGIN inside the shell
        else:
            d = rng.uniform(shell + MARGIN + 0.01, 0.75)            # >= MARGIN outside
        R = d + rad + ORAD
        far_r.append(0.0 if i in inside else R)
        c = START + R * u
        rows.append([c[0], c[1], c[2], 0.0, 0.0, 0.0, ORAD])
    if moving and K < M:
        mv = int(np.argmax(far_r))
        assert mv not in inside
        rows[mv][3:6] = list(MOVER_VEL)      # x, y away from the start; the list is handed to every tick unadvanced
        assert np.dot(MOVER_VEL, np.asarray(rows[mv][0:3]) - START) > 0
    elif moving:
        # K = M leaves no far obstacle: the holder nearest the middle of the shell moves instead -- 4.4 mm in a rollout
        # of eight steps, well inside the margin (the list is handed to every tick unadvanced)
        ds = [np.linalg.norm(np.asarray(r[0:3]) - START) - (rad + ORAD) for r in rows]
        mv = int(np.argmin(np.abs(np.asarray(ds) - 0.2)))
        rows[mv][3:6] = list(MOVER_VEL)
        assert MARGIN + 0.03 < ds[mv] < shell - MARGIN - 0.03, ds[mv]
    if sent_near:
        rows.append(list(START + np.array([-0.05, 0.3, 0.0])) + [0.0, 0.0, 0.0, SENT_RADIUS])
    else:
        rows.append([100.0, 100.0, 100.0, 0.0, 0.0, 0.0, SENT_RADIUS])
    obs = np.asarray(rows, dtype=np.float64)
    rv = rng.uniform(-1.0, 1.0, (N_AGENTS, M + 1, 3))
    rv /= np.linalg.norm(rv, axis=-1, keepdims=True)
    return dict(name="sum_chunks_K%d%s%s" % (K, "_moving" if moving else "", "_sent" if sent_near else ""),
                n_agents=N_AGENTS, max_prediction_steps=CAP, dt=0.01, velocity_max=0.2, approach_dist=0.25,
                detect_shell_rad=shell, agent_mass=1.0, radius=rad, k_attr=4.0, k_circ=0.025, k_repel=0.08, k_damp=3.0,
                cost_gains=np.array([100.0, 10.0, 0.001, 1.0]), ws_limits=np.array([1.0, -1.0, 0.3, -0.3, 1.1, 0.2]),
                start=START.copy(), goal=GOAL.copy(), obstacles=obs, random_vecs=rv,
                agent_types=scenes.default_agent_types(N_AGENTS))    # Had, Goal, Obstacle, GoalObstacle, Vel, Random x 2


def cases():
    """(K, moving, sent_near) of the plain handles"""
    return [(K, mv, sn) for K in KS for mv in (False, True) for sn in (False, True)]


def prepare(planner):
    """put a fresh planner (created with mgr_init_pos = INIT) at the start of the first tick"""
    planner.set_real_position(START)


def terms_at(sc, p, v, init_pos, margin=0.0):
    """indices of the field obstacles that give a term at position p with velocity v, by the geometry of circForce
    (cf_agent.cpp:76-98) and the gate (:315-317); margin: how far inside (> 0) the shell an obstacle has to be"""
    p, v = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
    g = sc["goal"] - p
    dg = np.linalg.norm(g)
    if dg < sc["approach_dist"] or (np.linalg.norm(v) < 0.5 * sc["velocity_max"] and np.linalg.norm(p - init_pos) < 0.2):
        return []
    out = []
    for i, o in enumerate(sc["obstacles"][:-1]):
        ro = o[0:3] - p
        rv = v - o[3:6]
        s = np.linalg.norm(ro)
        if np.dot(ro / s, g / dg) < -0.01 and np.dot(ro, rv) < -0.01:
            continue
        d = max(s - (sc["radius"] + o[6]), 1e-5)
        if d < sc["detect_shell_rad"] - margin and np.dot(rv, rv) != 0.0:
            out.append(i)
    return out
