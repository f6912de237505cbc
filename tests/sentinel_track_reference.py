"""Reference of the repulsive track (include/pmaf.h "repulsive track") at tolerance 0, composed from the oracle's existing
stepping API, and the cases tests/test_sentinel_track.py (CPU) and tests/test_sentinel_track_gpu.py (device) share.

The oracle's plan_steps (orc_move_agent(..., steps=1, id, max_calls=1)) is prediction_step's body with the CALLER's obstacle
list and no obstacle advance. A tracked rollout of agent i is therefore, after the agents were (re)set: while
sqrt(dot(g - p)) > 0.1 and n < cap -- the dot product in the build's association, exact IEEE in Python floats -- one
such call with the field obstacles at their iterated positions (o += v * dt in float64 numpy: multiply, then add), the
trailing one at y_{min(k, L-1)}, and the radii of the handle's creation list (resetEEAgents does not copy radii).
`reached` is dist < 0.100001 if any step ran. Costs come from orc_evaluate. With the straight-line track -- or none --
the composer IS orc_rollout, which tests/test_sentinel_track.py shows bit for bit on every case below.

Test infrastructure: imports neither the package nor the oracle; both are handed in."""
import math

import numpy as np

MUTANTS = ("ignore", "kplus", "kminus", "nohold", "field_static", "radius")


def goal_dist(order, g, p):
    d = [float(g[c]) - float(p[c]) for c in range(3)]
    s = [x * x for x in d]
    z = (s[0] + s[1]) + s[2] if order == 0 else s[0] + (s[1] + s[2])
    return math.sqrt(z)


def track_point(track, k, mutant=None):
    """y_{min(k, L-1)}; None where the (mutant) rule falls back to the straight line"""
    L = len(track)
    if mutant == "kplus":
        k = k + 1
    elif mutant == "kminus":
        k = max(k - 1, 0)
    if mutant == "nohold" and k > L - 1:
        return None
    return track[min(k, L - 1)]


def compose(ora, order, sc, obs0, track, mutant=None, agents=None):
    """Roll every agent of the oracle planner `ora` (already set / reset: its agents hold obs0's positions and
    velocities) out against `track` ([L][3], None or L == 0: untracked). Returns the rollout's results; the oracle's
    agents hold the paths afterwards (orc_evaluate scores them)."""
    N, cap = ora.N, ora.cap
    M = ora.n_obs - 1
    dt = float(sc["dt"])
    goal = np.asarray(sc["goal"], dtype=np.float64)
    radii = np.asarray(sc["obstacles"], dtype=np.float64)[:, 6]
    use_track = track is not None and len(track) > 0 and mutant != "ignore"
    reached = np.asarray(ora.success()).copy()
    for i in (range(N) if agents is None else agents):
        obs = np.array(obs0, dtype=np.float64).reshape(M + 1, 7).copy()
        obs[:, 6] = radii
        if mutant == "radius":
            obs[M, 6] = radii[M] + 0.03
        paths, n = ora.paths()
        p, n_i = paths[i, n[i] - 1], int(n[i])
        k, ran = 0, False
        while goal_dist(order, goal, p) > 0.1 and n_i < cap:
            lst = obs.copy()
            if use_track:
                y = track_point(track, k, mutant)
                if y is not None:
                    lst[M, 0:3] = y
            assert ora.move_agent(lst, dt, 1, i, max_calls=1) == 1
            if mutant != "field_static":
                obs[:M, 0:3] = obs[:M, 0:3] + obs[:M, 3:6] * dt
            obs[M, 0:3] = obs[M, 0:3] + obs[M, 3:6] * dt
            paths, n = ora.paths()
            assert n[i] == n_i + 1
            n_i += 1
            p = paths[i, n_i - 1]
            k += 1
            ran = True
        if ran:
            reached[i] = 1 if goal_dist(order, goal, p) < 0.100001 else 0
    paths, n = ora.paths()
    return dict(paths=paths, n_points=n, min_obs=ora.min_obs_dist(), known=ora.known(), rot=ora.rot_vecs(),
                vel=ora.agent_vel(), reached=reached)


def straight_line(obs0, dt, n):
    """the iterated o_M + k v_M dt of the untracked rollout, n points, bit for bit (multiply, then add)"""
    o = np.asarray(obs0, dtype=np.float64)[-1]
    y = np.zeros((n, 3))
    q = o[0:3].copy()
    for k in range(n):
        y[k] = q
        q = q + o[3:6] * dt
    return y


def coupled_track(path, n_points, has_best, shift):
    """pmaf_couple_tracks' rule on one selected path: [max(n - shift, 1)][3] from point `shift` on (a path of no more
    than `shift` points: its last point alone); no selection yet: no track"""
    if not has_best:
        return np.zeros((0, 3))
    n = int(n_points)
    first = min(int(shift), n - 1)
    return np.array(path[first:n], dtype=np.float64)


# ---- cases ------------------------------------------------------------------------------------------------------------
# name -> dict(M, cap, moving, mass, k_attr0, env): the smallest shapes that reach every branch of k_rollout_w64_track --
#   M = 3 / 59 / 60    few obstacles; the rel_vel rider in lane 59 beside the obstacle in lane 60; lane 59 taken (no rider
#                      while the obstacle is in reach)
#   cap 9 / 70         a rollout shorter than most tracks / one that moves 0.14 m: the track enters and leaves the range
#   moving             one field obstacle moves: the loops without the rel_vel rider
#   general            mass != 1 and one agent with k_attr == 0: the general step
#   lds                the LDS-batch ordered sum (PMAF_SUM=lds at create)
N_AGENTS = 7     # the six heuristics (the default layout's five + Random) and a second Random agent
SHAPES = {
    "M3-cap9": dict(M=3, cap=9),
    "M3-cap70": dict(M=3, cap=70),
    "M59-cap70": dict(M=59, cap=70),
    "M60-cap70": dict(M=60, cap=70),
    "M3-cap70-moving": dict(M=3, cap=70, moving=True),
    "M59-cap70-moving": dict(M=59, cap=70, moving=True),
    "M3-cap70-general": dict(M=3, cap=70, general=True),
    "M59-cap9-general-moving": dict(M=59, cap=9, general=True, moving=True),
    "M3-cap70-lds": dict(M=3, cap=70, env={"PMAF_SUM": "lds"}),
    "M60-cap70-lds-general-moving": dict(M=60, cap=70, general=True, moving=True, env={"PMAF_SUM": "lds"}),
}
SENT_RADIUS = 0.1


def build_scene(scenes, shape, scene_id=0):
    s = SHAPES[shape]
    sc = scenes.synthetic_scene(N_AGENTS, s["cap"] - 1, s["M"], config_id=11, scene_id=scene_id, dynamic=False)
    if s.get("moving"):
        sc["obstacles"][1, 3:6] = [0.04, -0.03, 0.02]
    sc["k_attr"] = np.linspace(3.0, 5.0, N_AGENTS)
    sc["k_repel"] = np.linspace(0.06, 0.1, N_AGENTS)
    if s.get("general"):
        sc["agent_mass"] = 1.25
        sc["k_attr"][2] = 0.0
    # the untracked obstacle: a sphere beside the start that drifts away, in range at first
    at = sc["start"] + np.array([0.05, 0.3 + 0.02 * scene_id, 0.02])
    sc["obstacles"][-1] = [at[0], at[1], at[2], 0.3, 0.6, -0.2, SENT_RADIUS]
    return sc


def in_range(sc, p, y):
    """repelForce's range test for one position pair, as the reference writes it"""
    d = math.sqrt(sum((float(p[c]) - float(y[c])) ** 2 for c in range(3))) - (sc["radius"] + SENT_RADIUS)
    return max(d, 1e-5) < sc["detect_shell_rad"]


def tracks_for(sc, ref_path, ref_n):
    """name -> track [L][3] for a scene, from the UNTRACKED oracle path of agent 0 (ref_path [cap][3], ref_n points):
       L1, L2, Lcap, Lcap+5    the lengths' edges (beside the agent: in range)
       short                   shorter than the rollout: the held end
       in_out                  0.56 m from the path for a third of it, 0.3 m, then 0.6 m: the range test goes both ways
       far                     beyond the reach bound everywhere: the loop without code for the obstacle
       on_start                one point exactly on the start position (the distance floor 1e-5)"""
    cap = int(sc["max_prediction_steps"])
    path = np.array(ref_path[:ref_n], dtype=np.float64)
    ext = np.concatenate([path, np.repeat(path[-1:], cap + 5 - len(path), axis=0)]) if len(path) < cap + 5 else path
    side = np.array([0.0, 1.0, 0.0])
    k = np.arange(cap + 5)
    wob = np.stack([0.01 * np.sin(0.7 * k), 0.02 * np.cos(0.3 * k), 0.015 * np.sin(0.2 * k + 1.0)], axis=1)
    near = ext + 0.3 * side + wob
    third = max(1, (ref_n - 1) // 3)
    off = np.where(k < third, 0.56, np.where(k < 2 * third, 0.3, 0.6))
    in_out = ext + off[:, None] * side + 0.2 * wob
    on_start = near[:max(4, cap // 2)].copy()
    on_start[min(2, len(on_start) - 1)] = sc["start"]
    return {
        "L1": near[:1], "L2": near[:2], "Lcap": near[:cap], "Lcap+5": near[:cap + 5],
        "short": near[:max(2, (ref_n - 1) // 2)],
        "in_out": in_out[:cap],
        "far": ext[:cap] + np.array([0.0, 30.0, 0.0]),
        "on_start": on_start,
    }


TRACKS = ("L1", "L2", "Lcap", "Lcap+5", "short", "in_out", "far", "on_start")
# the tracks every shape runs; the first shape of each group of SHAPE_GROUPS runs them all
CORE_TRACKS = ("L2", "short", "in_out", "far")
SHAPE_GROUPS = {
    "plain-dpp": ("M3-cap70", "M3-cap9", "M59-cap70", "M60-cap70", "M3-cap70-moving", "M59-cap70-moving"),
    "general": ("M3-cap70-general", "M59-cap9-general-moving"),
    "lds": ("M3-cap70-lds", "M60-cap70-lds-general-moving"),
}


def case_list():
    out = []
    for group, shapes in SHAPE_GROUPS.items():
        for j, sh in enumerate(shapes):
            for t in (TRACKS if j == 0 else CORE_TRACKS):
                out.append((sh, t))
    return out


# ---- coupled ticks ------------------------------------------------------------------------------------------------------
def dual_scenes(scenes, shape="M3-cap70"):
    """two arms 0.25 m apart whose goals are swapped in y: each arm's selected path is inside the other's repel range"""
    scs = []
    for p in range(2):
        sc = build_scene(scenes, shape, scene_id=p)
        sc["start"] = sc["start"] + np.array([0.0, 0.25 * p - 0.125, 0.0])
        sc["goal"] = sc["goal"] + np.array([0.0, 0.125 - 0.25 * p, 0.0])
        # the live list's sphere rests at the other arm's start, as DualArmCoupling leaves it at the last set-point
        other = np.array([-0.6, 0.125 - 0.25 * p, 0.7])
        sc["obstacles"][-1] = [other[0], other[1], other[2], 0.0, 0.0, 0.0, SENT_RADIUS]
        if p == 0:      # the arms select different agent indices (far from the goal the damping decides, not k_attr)
            sc["k_damp"] = np.linspace(2.0, 4.0, N_AGENTS)
        scs.append(sc)
    return scs


def coupled_ticks(orc, scs, src_pop, shift, n_ticks):
    """The planCallback sequence of P oracle planners whose rollouts follow each other's selected paths
    (pmaf_couple_tracks): per tick every planner selects, then -- from the paths as they lie after every selection --
    population p takes coupled_track(selected path of src_pop[p]); real step, reset and the composed rollout follow.
    src_pop None: uncoupled. Returns the first rollout's results and per tick (best [P], tracks [P], results [P])."""
    order = orc.eval_order()
    P = len(scs)
    oras = [orc.OraclePlanner(sc, mgr_init_pos=sc["start"]) for sc in scs]
    first = []
    for ora, sc in zip(oras, scs):
        ora.set_initial_position(sc["start"])
        first.append(compose(ora, order, sc, sc["obstacles"], None))     # no selection yet: untracked
    ticks = []
    for t in range(n_ticks):
        best = [ora.evaluate(sc["cost_gains"], sc["ws_limits"]) for ora, sc in zip(oras, scs)]
        sel = []
        for ora, b in zip(oras, best):
            paths, n = ora.paths()
            sel.append((paths[b].copy(), int(n[b])))
        tracks, res = [], []
        for p, (ora, sc) in enumerate(zip(oras, scs)):
            q = -1 if src_pop is None else src_pop[p]
            tr = coupled_track(sel[q][0], sel[q][1], True, shift) if q >= 0 else np.zeros((0, 3))
            ora.move_real(sc["obstacles"], sc["dt"], 1, best[p])
            pos, vel, _ = ora.real_state()
            ora.reset_agents(pos, vel, sc["obstacles"])
            tracks.append(tr)
            res.append(compose(ora, order, sc, sc["obstacles"], tr))
        ticks.append((best, tracks, res))
    return first, ticks
