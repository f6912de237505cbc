"""Reference of the obstacle tracks (include/pmaf.h "obstacle tracks") at tolerance 0: the composer of
tests/sentinel_track_reference.py -- one orc_move_agent(steps=1, max_calls=1) per prediction step with the caller's
list -- extended from the trailing obstacle to the M field obstacles, and the cases tests/test_field_track.py (CPU) and
tests/test_field_track_gpu.py (device) share.

Per step k the list handed to the oracle has, in rows 0 ... M-1, columns 0:6 (position AND velocity) of point
min(first + k, L-1) of the tracks, the radii of the creation list, and in the trailing row what the repulsive track's
composer puts there: y_{min(k, L'-1)} of a repulsive track, else the iterated o_M + k v_M dt. With the iterated straight
lines and the constant velocities as tracks the composer IS orc_rollout, which tests/test_field_track.py shows bit for bit.

Test infrastructure: imports neither the package nor the oracle; both are handed in."""
import numpy as np

import sentinel_track_reference as ref

MUTANTS = ("ignore", "kplus", "kminus", "nohold", "posonly", "first_ignored", "trailing", "radius")
N_AGENTS = ref.N_AGENTS
SHAPES = ref.SHAPES
SHAPE_GROUPS = ref.SHAPE_GROUPS
build_scene = ref.build_scene


def field_point(tracks, first, k, mutant=None):
    """point min(first + k, L-1) of tracks [L][M][6]; None where the (mutant) rule falls back to the straight lines"""
    L = len(tracks)
    idx = (0 if mutant == "first_ignored" else int(first)) + k
    if mutant == "kplus":
        idx += 1
    elif mutant == "kminus":
        idx = max(idx - 1, 0)
    if mutant == "nohold" and idx > L - 1:
        return None
    return tracks[min(idx, L - 1)]


def compose(ora, order, sc, obs0, ftracks, first=0, track=None, mutant=None, agents=None):
    """Roll every agent of the oracle planner `ora` (already set / reset: its agents hold obs0's positions and
    velocities) out against the obstacle tracks `ftracks` ([L][M][6]; None or L == 0: none) from offset `first`, and the
    repulsive track `track` ([L'][3] or None). Returns the rollout's results; the oracle's agents hold the paths."""
    N, cap = ora.N, ora.cap
    M = ora.n_obs - 1
    dt = float(sc["dt"])
    goal = np.asarray(sc["goal"], dtype=np.float64)
    radii = np.asarray(sc["obstacles"], dtype=np.float64)[:, 6]
    use_f = ftracks is not None and len(ftracks) > 0 and mutant != "ignore"
    use_t = track is not None and len(track) > 0
    if use_f:
        ftracks = np.asarray(ftracks, dtype=np.float64).reshape(len(ftracks), -1, 6)[:, :M]
    reached = np.asarray(ora.success()).copy()
    for i in (range(N) if agents is None else agents):
        obs = np.array(obs0, dtype=np.float64).reshape(M + 1, 7).copy()
        obs[:, 6] = radii
        paths, n = ora.paths()
        p, n_i = paths[i, n[i] - 1], int(n[i])
        k, ran = 0, False
        while ref.goal_dist(order, goal, p) > 0.1 and n_i < cap:
            lst = obs.copy()
            if use_t:
                lst[M, 0:3] = ref.track_point(track, k)
            if use_f:
                pt = field_point(ftracks, first, k, mutant)
                if pt is not None:
                    if mutant == "posonly":
                        lst[:M, 0:3] = pt[:, 0:3]
                    else:
                        lst[:M, 0:6] = pt
                    if mutant == "trailing":
                        lst[M, 0:6] = pt[M - 1]
                if mutant == "radius":
                    lst[:M, 6] = radii[:M] + 0.03
            assert ora.move_agent(lst, dt, 1, i, max_calls=1) == 1
            obs[:, 0:3] = obs[:, 0:3] + obs[:, 3:6] * dt
            paths, n = ora.paths()
            assert n[i] == n_i + 1
            n_i += 1
            p = paths[i, n_i - 1]
            k += 1
            ran = True
        if ran:
            reached[i] = 1 if ref.goal_dist(order, goal, p) < 0.100001 else 0
    paths, n = ora.paths()
    return dict(paths=paths, n_points=n, min_obs=ora.min_obs_dist(), known=ora.known(), rot=ora.rot_vecs(),
                vel=ora.agent_vel(), reached=reached)


def straight_lines(obs0, dt, n):
    """the iterated o_i + k v_i dt of the untracked rollout with the constant velocities, [n][M][6], bit for bit
    (multiply, then add)"""
    o = np.asarray(obs0, dtype=np.float64)[:-1]
    out = np.zeros((n, len(o), 6))
    q = o[:, 0:3].copy()
    for k in range(n):
        out[k, :, 0:3] = q
        out[k, :, 3:6] = o[:, 3:6]
        q = q + o[:, 3:6] * dt
    return out


def tracks_for(sc, ref_path, ref_n):
    """name -> tracks [L][M][6] for a scene, from the UNTRACKED oracle path of agent 0 (ref_path [cap][3], ref_n points).
    Every obstacle leaves its straight line a little (a slow drift with a velocity of its own), and two of them -- the
    first and the last, lanes 0 and M-1 -- travel with the agents:
       L1, L2, Lcap, Lcap+5    the lengths' edges; obstacle 0 0.25 m beside the path (inside the shell), M-1 below it
       short                   shorter than the rollout: the held end
       sweep                   obstacle 0 comes from 0.6 m (outside the shell) across to 0.22 m and leaves again, obstacle
                               M-1 the other way round: the latch happens on a tracked position, mid-rollout
       line                    the straight lines (the untracked rollout's bits)"""
    cap = int(sc["max_prediction_steps"])
    dt = float(sc["dt"])
    M = len(sc["obstacles"]) - 1
    K = cap + 5
    path = np.array(ref_path[:ref_n], dtype=np.float64)
    ext = np.concatenate([path, np.repeat(path[-1:], K - len(path), axis=0)]) if len(path) < K else path[:K]
    k = np.arange(K)
    line = straight_lines(sc["obstacles"], dt, K)
    side, down = np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, -1.0])
    wob = np.stack([0.01 * np.sin(0.7 * k), 0.02 * np.cos(0.3 * k), 0.015 * np.sin(0.2 * k + 1.0)], axis=1)

    def with_travellers(off0, off1):
        t = line.copy()
        # every obstacle: a drift off the line and a velocity that is not the list's
        i = np.arange(M)[None, :, None]
        t[:, :, 0:3] += 0.0004 * k[:, None, None] * np.cos(i + np.arange(3)[None, None, :])
        t[:, :, 3:6] += 0.03 * np.sin(0.1 * k[:, None, None] + i + np.arange(3)[None, None, :])
        t[:, 0, 0:3] = ext + off0[:, None] * side + wob
        t[:, 0, 3:6] = np.stack([0.2 * np.cos(0.05 * k), -0.5 + 0.01 * k, 0.1 * np.sin(0.3 * k)], axis=1)
        t[:, M - 1, 0:3] = ext + off1[:, None] * down - 0.5 * wob
        t[:, M - 1, 3:6] = np.stack([0.1 * np.sin(0.2 * k), 0.05 * np.cos(0.1 * k), 0.4 - 0.01 * k], axis=1)
        return t

    near = with_travellers(np.full(K, 0.25), np.full(K, 0.3))
    third = max(1, (ref_n - 1) // 3)
    ramp = np.clip(np.abs(k - 1.5 * third) / (1.5 * third), 0.0, 1.0)      # 1 -> 0 -> 1 over the rollout
    sweep = with_travellers(0.22 + 0.38 * ramp, 0.6 - 0.36 * ramp)
    return {
        "L1": near[:1], "L2": near[:2], "Lcap": near[:cap], "Lcap+5": near[:cap + 5],
        "short": near[:max(2, (ref_n - 1) // 2)],
        "sweep": sweep[:cap],
        "line": line[:cap],
    }


def tracked_ticks(orc, sc, ftracks, n_ticks, advance=1):
    """The planCallback sequence of one oracle planner whose rollouts follow `ftracks` one point further every tick
    (pmaf_set_obstacle_track_offset): the first rollout from offset 0, then per tick select, real step against the live
    list, reset, and the composed rollout from offset advance * (t + 1). Returns the first rollout's results and per tick (best, results)."""
    order = orc.eval_order()
    ora = orc.OraclePlanner(sc, mgr_init_pos=sc["start"])
    ora.set_initial_position(sc["start"])
    first = compose(ora, order, sc, sc["obstacles"], ftracks, 0)
    ticks = []
    for t in range(n_ticks):
        best = ora.evaluate(sc["cost_gains"], sc["ws_limits"])
        ora.move_real(sc["obstacles"], sc["dt"], 1, best)
        pos, vel, _ = ora.real_state()
        ora.reset_agents(pos, vel, sc["obstacles"])
        ticks.append((best, compose(ora, order, sc, sc["obstacles"], ftracks, advance * (t + 1))))
    return first, ticks


def shell_distance(sc, p, o, r):
    return float(np.linalg.norm(np.asarray(p) - np.asarray(o))) - (sc["radius"] + r)


# (tracks name, first): `first` as a number, or "L-1" / "L+3" resolved against the track's length
ALL_CASES = (("L1", 0), ("L2", 0), ("L2", 1), ("Lcap", 0), ("Lcap", 1), ("Lcap+5", 0), ("short", 0), ("short", "L-1"),
             ("short", "L+3"), ("sweep", 0), ("sweep", 1))
CORE_CASES = (("short", 0), ("Lcap", 1), ("sweep", 0))


def resolve_first(first, L):
    return {"L-1": L - 1, "L+3": L + 3}.get(first, first)


def case_list():
    """(shape, tracks name, first): the first shape of each group runs every case, the others the core"""
    out = []
    for group, shapes in SHAPE_GROUPS.items():
        for j, sh in enumerate(shapes):
            for t, f in (ALL_CASES if j == 0 else CORE_CASES):
                out.append((sh, t, f))
    return out
