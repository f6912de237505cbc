"""Exact-tie scenes: dyadic and Pythagorean geometry in which the strict arithmetic policies compute the tied quantities
exactly, so the high-precision reference (tests/hp_reference.py) decides each tie with bound 0 and a planner must take
the same side. Each scene is driven through the planner's own C-ABI surface and shadowed (tests/hp_shadow.py); its
`tie` re-evaluates the tied comparison in the reference and requires it to be exact.

Shared by the oracle test (tests/test_hp_reference.py) and the kernel test (tests/test_hp_reference_gpu.py).
"""
import numpy as np

import hp_reference as hp
import hp_shadow as sh

P0 = np.array([0.25, 0.25, 0.5])
FAR = [2.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0625]          # a field obstacle out of every shell
SENTINEL = [100.0, 100.0, 100.0, 0.0, 0.0, 0.0, 0.1]
ALL_TYPES = [hp.HAD, hp.GOAL, hp.OBSTACLE, hp.GOAL_OBSTACLE, hp.VEL, hp.RANDOM]


def edge_scene(obstacles, goal, cap=2, types=ALL_TYPES, **over):
    n = len(types)
    rng = np.random.default_rng(3)
    rv = rng.uniform(-1, 1, (n, len(obstacles), 3))
    rv /= np.linalg.norm(rv, axis=-1, keepdims=True)
    s = dict(name="edge", n_agents=n, max_prediction_steps=cap, dt=0.0625, velocity_max=0.25, approach_dist=0.25,
             detect_shell_rad=0.375, agent_mass=1.0, radius=0.0625, k_attr=4.0, k_circ=0.03125, k_repel=0.0625,
             k_damp=4.0, cost_gains=np.array([100.0, 10.0, 0.001, 1.0]),
             ws_limits=np.array([1.0, -1.0, 1.0, -1.0, 2.0, 0.0]), start=P0.copy(), goal=np.asarray(goal, dtype=float),
             obstacles=np.asarray(obstacles, dtype=np.float64), random_vecs=rv,
             agent_types=np.asarray(types, dtype=np.int32))
    s.update(over)
    return s


class Edge:
    def __init__(self, name, scene, drive, tie):
        self.name, self.scene, self.drive, self.tie = name, scene, drive, tie
        self.tie_seen = False

    def run(self, make_planner, A, st):
        sc = self.scene
        pl = make_planner(sc)
        try:
            self.drive(pl, sc, A, st)
        finally:
            pl.close()
        self.tie(A, sc)
        self.tie_seen = True


def _steps(pos, vel, init, evaluate=False):
    def drive(pl, sc, A, st):
        pl.set_initial_position(init)
        pl.set_agent_pos_and_vels(pos, vel)
        sh.shadow_steps(pl, sc, sc["obstacles"], np.asarray(init, dtype=float), A, st, 1)
        if evaluate:
            sh.shadow_evaluate(pl, sc, A, st)
    return drive


def _rollout(pos, vel, init, evaluate=False, best=None):
    def drive(pl, sc, A, st):
        pl.set_initial_position(init)
        sh.shadow_reset_rollout(pl, sc, pos, vel, sc["obstacles"], np.asarray(init, dtype=float), A, st)
        if best is not None:
            pl.set_best(best[0], best[1], sc["random_vecs"][best[0] - 1])
        if evaluate:
            sh.shadow_evaluate(pl, sc, A, st)
    return drive


def _exact_equal(q, x, A):
    assert q.e == 0.0 and q.v == A.c(x).v, (q, x)


def _dist(A, p, row, rad):
    return A.sub(A.norm(A.vsub(A.v3(row[:3]), A.v3(p))), A.add(A.c(rad), A.c(row[6])))


# obstacle surface exactly at the shell: |(0.375, 0.5, 0)| = 0.625, radii 0.0625 + 0.1875, shell 0.375
_shell_obs = [list(P0 + [0.375, 0.5, 0.0]) + [0.0, 0.0, 0.0, 0.1875],
              list(P0 + [0.25, -0.25, 0.0]) + [0.0, 0.0, 0.0, 0.0625], SENTINEL]
E_SHELL = Edge("obstacle at exactly the shell distance",
               edge_scene(_shell_obs, P0 + [1.0, 0.0, 0.0]),
               _steps(P0, [0.125, 0.0, 0.0], P0 - [0.0, 0.0, 0.5]),
               lambda A, sc: _exact_equal(_dist(A, P0, sc["obstacles"][0], 0.0625), 0.375, A))
# ... and in a rollout (the rollout kernels' shell test, not the stepping kernel's)
E_SHELL_ROLL = Edge("obstacle at exactly the shell distance, rollout",
                    edge_scene(_shell_obs, P0 + [1.0, 0.0, 0.0]),
                    _rollout(P0, [0.125, 0.0, 0.0], P0 - [0.0, 0.0, 0.5]),
                    lambda A, sc: _exact_equal(_dist(A, P0, sc["obstacles"][0], 0.0625), 0.375, A))

# |a| = 13 exactly: force 16 (goal_vec - 0) = (5, 12, 0); |vel_des| = vel_max (min(1, 1)); |v'| = |a dt| = vel_max
_acc_goal = P0 + [0.3125, 0.75, 0.0]
E_ACC = Edge("|a| = 13, |v| = vel_max and vel_max / |vel_des| = 1 exactly",
             edge_scene([FAR, SENTINEL], _acc_goal, velocity_max=0.8125, k_attr=16.0, k_damp=16.0),
             _steps(P0, [0.0, 0.0, 0.0], P0, evaluate=True),
             lambda A, sc: (_exact_equal(A.norm(A.v3([5.0, 12.0, 0.0])), 13.0, A),
                            _exact_equal(A.norm(A.v3([0.3125, 0.75, 0.0])), 0.8125, A)))

# the same, a hair above 13: the clamp acts
E_ACC_OVER = Edge("|a| just above 13",
                  edge_scene([FAR, SENTINEL], P0 + [0.3125, 0.75 + 2.0 ** -20, 0.0], velocity_max=1.0, k_attr=16.0,
                             k_damp=16.0),
                  _steps(P0, [0.0, 0.0, 0.0], P0),
                  lambda A, sc: None)

# the goal guard: goal exactly 0.1 away (axis-aligned: sqrt(fl(x * x)) = |x|) -> no step; 0.11 away -> one step, reached
_g = np.array([0.1, 0.25, 0.75])
E_GUARD = Edge("goal offset exactly 0.1",
               edge_scene([FAR, SENTINEL], _g),
               _rollout(np.array([0.0, 0.25, 0.75]), [0.375, 0.0, 0.0], np.array([0.0, 0.25, 0.25]), evaluate=True),
               lambda A, sc: _exact_equal(A.norm(A.vsub(A.v3(_g), A.v3([0.0, 0.25, 0.75]))), 0.1, A))
E_REACHED = Edge("goal reached within one step",
                 edge_scene([FAR, SENTINEL], _g, cap=8),
                 _rollout(np.array([-0.015625, 0.25, 0.75]), [0.25, 0.0, 0.0], np.array([0.0, 0.25, 0.25])),
                 lambda A, sc: None)

# overlapping spheres: the 1e-5 floor, min_obs_dist = 1e-5 < 2e-5 (cost penalty), a clamped acceleration
E_FLOOR = Edge("overlapping spheres",
               edge_scene([list(P0 + [0.0625, 0.03125, 0.0]) + [0.0, 0.0, 0.0, 0.125], FAR, SENTINEL],
                          P0 + [1.0, 0.0, 0.0]),
               _rollout(P0, [0.125, 0.0, 0.0], P0 - [0.0, 0.0, 0.5]),
               lambda A, sc: None)
# ... evaluated: identical heuristics, so the costs tie exactly
E_FLOOR_COST = Edge("overlapping spheres, cost penalty",
                    edge_scene([list(P0 + [0.0625, 0.03125, 0.0]) + [0.0, 0.0, 0.0, 0.125], FAR, SENTINEL],
                               P0 + [1.0, 0.0, 0.0], types=[hp.GOAL, hp.GOAL, hp.GOAL]),
                    _rollout(P0, [0.125, 0.0, 0.0], P0 - [0.0, 0.0, 0.5], evaluate=True),
                    lambda A, sc: None)

# an obstacle moving with the agent: relative velocity exactly 0
E_RELVEL = Edge("obstacle at the agent's velocity",
                edge_scene([list(P0 + [0.25, 0.125, 0.0]) + [0.125, 0.0, 0.0, 0.0625], FAR, SENTINEL],
                           P0 + [1.0, 0.0, 0.0]),
                _steps(P0, [0.125, 0.0, 0.0], P0 - [0.0, 0.0, 0.5]),
                lambda A, sc: _exact_equal(A.norm(A.vsub(A.v3([0.125, 0.0, 0.0]), A.v3(sc["obstacles"][0][3:6]))), 0.0, A))

# an obstacle on the goal line, the agent moving along it: degenerate goal / velocity currents (Had's rotation vector
# is 0 / 0 there -- a NaN in the reference too -- so the population leaves it out)
E_LINE = Edge("obstacle on the goal line",
              edge_scene([list(P0 + [0.25, 0.0, 0.0]) + [0.0, 0.0, 0.0, 0.0625],
                          list(P0 + [0.5, 0.25, 0.0]) + [0.0, 0.0, 0.0, 0.0625], SENTINEL], P0 + [1.0, 0.0, 0.0],
                         types=[hp.GOAL, hp.OBSTACLE, hp.GOAL_OBSTACLE, hp.VEL, hp.RANDOM]),
              _steps(P0, [0.125, 0.0, 0.0], P0 - [0.0, 0.0, 0.5]),
              lambda A, sc: None)

# path points exactly on a workspace limit (x = xmax = 1.0, moving along y), and beyond zmax
E_WS = Edge("path on a workspace limit",
            edge_scene([FAR, SENTINEL], np.array([1.0, 1.25, 0.75]), ws_limits=np.array([1.0, -1.0, 1.0, -1.0, 0.5, 0.0])),
            _rollout(np.array([1.0, 0.25, 0.75]), [0.0, 0.125, 0.0], np.array([1.0, 0.25, 0.25]), evaluate=True),
            lambda A, sc: None)

# two obstacles at equal centre distance from the one entering the shell: first minimum
_o0 = P0 + [0.25, 0.125, 0.0]
E_CLOSEST = Edge("equal centre distances for closest_other",
                 edge_scene([list(_o0) + [0.0, 0.0, 0.0, 0.0625], list(_o0 + [0.25, 0.0, 0.0]) + [0.0, 0.0, 0.0, 0.0625],
                             list(_o0 + [0.0, 0.25, 0.0]) + [0.0, 0.0, 0.0, 0.0625], SENTINEL], P0 + [1.0, 0.0, 0.0]),
                 _steps(P0, [0.125, 0.0, 0.0], P0 - [0.0, 0.0, 0.5]),
                 lambda A, sc: _exact_equal(A.norm(A.vsub(A.v3(sc["obstacles"][1][:3]), A.v3(_o0))), 0.25, A))

# the hysteresis switches: best_agent_ is an agent without attraction (k_attr = 0: it stays), the other one's rollout
# ends far closer to the goal (cost 100 |g - p| + 10 length: about 48 against 100)
E_HYST = Edge("hysteresis switch",
              edge_scene([FAR, SENTINEL], P0 + [1.0, 0.0, 0.0], cap=8, types=[hp.GOAL, hp.GOAL], velocity_max=1.0,
                         k_attr=np.array([0.0, 16.0]), k_damp=16.0),
              _rollout(P0, [0.0, 0.0, 0.0], P0, evaluate=True, best=(1, hp.GOAL)),
              lambda A, sc: None)

# the hysteresis at its edge: with only the path-length gain, one gate-closed step from rest costs k_attr * 2^-9 (goal
# straight along x, k_damp = 1, dt = 2^-4), so the costs stand in the ratio 0.90000005 : 1 -- just above the 0.9 factor
E_HYST_EDGE = Edge("costs just above the hysteresis factor",
                   edge_scene([FAR, SENTINEL], P0 + [1.0, 0.0, 0.0], types=[hp.GOAL, hp.GOAL], velocity_max=4.0,
                              k_attr=np.array([1.0, 0.90000005]), k_damp=1.0,
                              cost_gains=np.array([0.0, 1.0, 0.0, 0.0])),
                   _rollout(P0, [0.0, 0.0, 0.0], P0, evaluate=True, best=(1, hp.GOAL)),
                   lambda A, sc: None)

EDGES = [E_SHELL, E_SHELL_ROLL, E_ACC, E_ACC_OVER, E_GUARD, E_REACHED, E_FLOOR, E_FLOOR_COST, E_RELVEL, E_LINE, E_WS, E_CLOSEST, E_HYST, E_HYST_EDGE]
