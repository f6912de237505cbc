"""Reference of the obstacle tracks' device-side source (include/pmaf.h "obstacle tracks", pmaf_couple_obstacle_tracks) at
tolerance 0: the composition of a coupled population's tracks from the other populations' selected paths, every rounding
a separate numpy operation on float64, and the coupled tick sequence -- coupled_ticks of
tests/sentinel_track_reference.py with the composer of tests/field_track_reference.py -- that tests/test_field_couple.py
(CPU) and tests/test_field_couple_gpu.py (device) share.

Test infrastructure: imports neither the package nor the oracle; both are handed in."""
import numpy as np

import field_track_reference as fref
import sentinel_track_reference as sref

# each breaks one rule of the contract (tests/test_field_couple.py: every one changes path bits in every shape group)
MUTANTS = ("recip", "backward", "lastvel", "shift_ignored", "anchor_ignored", "scale_ignored", "agent0", "frozen", "novel")
N_AGENTS = sref.N_AGENTS
SHAPES = sref.SHAPES
SHAPE_GROUPS = sref.SHAPE_GROUPS


def compose_tracks(sel_paths, sel_n, has_best, src, scale, anchor, shift, obs_start, dt, cap, mutant=None):
    """The tracks [cap][M][6] ONE coupled population's rollout follows, or an empty array [0][M][6] (L = 0: no attached
    column whose source has a selection). sel_paths[q] / sel_n[q] / has_best[q]: the selected path ([>= n][3]), its
    point count and whether population q has a selection; src [M] (-1: unattached), scale [M], anchor [M][3]; obs_start
    [M+1][7] the rollout-start list; dt the rollout step."""
    obs_start = np.asarray(obs_start, dtype=np.float64)
    M = len(obs_start) - 1
    src = np.asarray(src, dtype=np.int64).reshape(M)
    scale = np.asarray(scale, dtype=np.float64).reshape(M)
    anchor = np.asarray(anchor, dtype=np.float64).reshape(M, 3)
    dt = np.float64(dt)
    live = [i for i in range(M) if src[i] >= 0 and has_best[src[i]]]
    if not live:
        return np.zeros((0, M, 6))
    out = fref.straight_lines(obs_start, dt, cap)        # unattached columns: q_{k+1} = RN(q_k + RN(v dt)), velocity v
    ncs = []
    for i in live:
        q = int(src[i])
        n = min(max(int(sel_n[q]), 1), cap)
        first = 0 if mutant == "shift_ignored" else min(int(shift), n - 1)
        y = np.array(sel_paths[q][first:n], dtype=np.float64)       # y_0 ... y_{n_c - 1}
        n_c = len(y)
        ncs.append(n_c)
        s = np.float64(1.0) if mutant == "scale_ignored" else scale[i]
        a = np.zeros(3) if mutant == "anchor_ignored" else anchor[i]
        prod = s * y                                                # RN(scale * y_k)
        x = a[None, :] + prod                                       # RN(anchor + .)
        u = np.zeros((n_c, 3))
        if n_c > 1:
            d = x[1:] - x[:-1]                                      # RN(x_{k+1} - x_k)
            if mutant == "recip":
                r = np.float64(1.0) / dt
                vel = d * r
            else:
                vel = d / dt                                        # the correctly rounded division
            if mutant == "backward":
                u[1:] = vel
            else:
                u[:-1] = vel                                        # +0.0 from k = n_c - 1 on
            if mutant == "lastvel":
                u[-1] = u[-2]
        k = np.minimum(np.arange(cap), n_c - 1)
        out[:, i, 0:3] = x[k]
        out[:, i, 3:6] = u[k]
    if mutant in ("frozen", "novel"):
        hold = max(ncs) - 1
        for i in range(M):
            if i in live:
                continue
            if mutant == "frozen":
                out[hold:, i, :] = out[hold, i, :]
            else:
                out[:, i, 3:6] = 0.0
    return out


def selected(oras, best, mutant=None):
    """every oracle planner's selected path as it lies after the selection: (paths [P], n [P])"""
    sel_p, sel_n = [], []
    for ora, b in zip(oras, best):
        paths, n = ora.paths()
        b = 0 if mutant == "agent0" else int(b)
        sel_p.append(paths[b].copy())
        sel_n.append(int(n[b]))
    return sel_p, sel_n


def field_coupled_ticks(orc, scs, src, scale, anchor, shift, n_ticks, repulsive_src=None, mutant=None, repulsive_shift=None,
                        uploaded=None, schedule=None):
    """The planCallback sequence of P oracle planners whose field obstacles ride on each other's selected paths
    (pmaf_couple_obstacle_tracks): sentinel_track_reference.coupled_ticks with field_track_reference.compose(...,
    ftracks=..., track=...). src [P][M] or None (uncoupled), scale [P][M], anchor [P][M][3]. repulsive_src [P] (or None):
    pmaf_couple_tracks on top, from point repulsive_shift (default: shift) on. Per tick every planner selects, then --
    from the paths as they lie after every selection -- population p's tracks are composed against the list its reset is
    about to write; real step, reset and the composed rollout follow. uploaded {p: (tracks, first)}: population p -- not
    a coupled one -- follows uploaded tracks from that offset instead (pmaf_set_obstacle_tracks). schedule: per tick
    (field coupling on, repulsive coupling on), for a caller that couples and uncouples between ticks; None: both as
    given, throughout. Returns the first rollout's results [P] (no selection yet: untracked but for uploaded tracks) and
    per tick (best [P], tracks [P], results [P])."""
    uploaded = uploaded or {}
    order = orc.eval_order()
    P = len(scs)
    oras = [orc.OraclePlanner(sc, mgr_init_pos=sc["start"]) for sc in scs]
    first = []
    for ora, sc in zip(oras, scs):
        ora.set_initial_position(sc["start"])
        up = uploaded.get(len(first), (None, 0))
        first.append(fref.compose(ora, order, sc, sc["obstacles"], up[0], up[1]))
    rshift = shift if repulsive_shift is None else repulsive_shift
    ticks = []
    for t in range(n_ticks):
        best = [ora.evaluate(sc["cost_gains"], sc["ws_limits"]) for ora, sc in zip(oras, scs)]
        sel_p, sel_n = selected(oras, best, mutant)
        true_p, true_n = selected(oras, best)
        tracks, res = [], []
        f_on, r_on = (True, True) if schedule is None else schedule[t]
        for p, (ora, sc) in enumerate(zip(oras, scs)):
            M = len(sc["obstacles"]) - 1
            cap = int(sc["max_prediction_steps"])
            f0 = 0
            if p in uploaded:
                ft, f0 = uploaded[p]
            elif src is None or not f_on:
                ft = np.zeros((0, M, 6))
            else:
                ft = compose_tracks(sel_p, sel_n, [True] * P, src[p], scale[p], anchor[p], shift, sc["obstacles"], sc["dt"], cap, mutant)
            q = -1 if repulsive_src is None or not r_on else repulsive_src[p]
            tr = sref.coupled_track(true_p[q], true_n[q], True, rshift) if q >= 0 else None
            ora.move_real(sc["obstacles"], sc["dt"], 1, best[p])
            pos, vel, _ = ora.real_state()
            ora.reset_agents(pos, vel, sc["obstacles"])
            tracks.append(ft)
            res.append(fref.compose(ora, order, sc, sc["obstacles"], ft, f0, tr))
        ticks.append((best, tracks, res))
    return first, ticks


def dual_scenes(scenes, shape="M3-cap70", short=False, moving=False):
    """sentinel_track_reference.dual_scenes for any shape, with arm 1 moved 0.58 m away (out of the range of the sphere
    at the other arm's last set-point, which otherwise drives the arms apart) and sent ACROSS arm 0's front: it travels
    -y while arm 0 travels +x, so what rides on one arm's path moves relative to the other arm -- a sphere beside it
    crosses the detection shell mid-rollout, and the arms come into each other's repel range. short = a distance (0.13;
    0.105 where the general step or a capacity of 9 would not get there): arm 1's goal lies that far from its start
    instead, so its selected path ends after a few points -- arm 0's attached columns are held there with velocity
    +0.0 while its unattached columns keep moving to the capacity"""
    scs = sref.dual_scenes(scenes, shape)
    if moving:      # (as build_scene's `moving`, for the shapes that come without: an unattached column that moves)
        for sc in scs:
            sc["obstacles"][1, 3:6] = [0.04, -0.03, 0.02]
    scs[1]["start"] = scs[0]["start"] + np.array([0.3, 0.5, 0.0])
    scs[1]["goal"] = scs[1]["start"] + np.array([0.0, -float(short) if short else -1.2, 0.0])
    for p in range(2):
        scs[p]["obstacles"][-1, 0:3] = scs[1 - p]["start"]
    return scs


def fast_scenes(scenes, shape="M3-cap70"):
    """sentinel_track_reference.dual_scenes as they are -- the arms flee each other's sphere at 2e-3 m per step -- moved
    0.115 m in y, so that arm 0's y passes through [0.008, 0.13]: there the difference of two neighbouring points keeps
    47 ... 50 significant bits, d * (1 / dt) = d * 100 rounds, and the reciprocal multiply differs from the division in
    some ten percent of that column's velocities (at 1e-4 m per step, or around |y| = 0.4, none does: the product is
    exact). The cases that hold the composed tracks' bits run on these."""
    scs = sref.dual_scenes(scenes, shape)
    for sc in scs:
        sc["start"] = sc["start"] + np.array([0.0, 0.115, 0.0])
        sc["goal"] = sc["goal"] + np.array([0.0, 0.115, 0.0])
        sc["obstacles"][:, 1] += 0.115
    return scs


def triple_scenes(scenes, shape="M3-cap70"):
    """three arms in one handle: population 0 between the other two; population 2's goal is 0.13 m from its start, so the
    two selected paths population 0's columns ride on have different lengths"""
    scs = dual_scenes(scenes, shape)
    sc = sref.build_scene(scenes, shape, scene_id=2)
    sc["start"] = scs[0]["start"] + np.array([0.3, -0.5, 0.0])
    sc["goal"] = sc["start"] + np.array([0.0, 0.13, 0.0])
    sc["obstacles"][-1] = scs[1]["obstacles"][-1]
    return scs + [sc]


# (shape, short, shift) per shape group, all with dual_scenes(moving=True): the tick sequences both suites run
GROUP_CASES = {
    "plain-dpp": (("M3-cap70-moving", False, 1), ("M3-cap70-moving", 0.13, 1), ("M59-cap70-moving", 0.13, 2)),
    "general": (("M3-cap70-general", False, 1), ("M3-cap70-general", 0.105, 1)),
    "lds": (("M60-cap70-lds-general-moving", False, 1), ("M60-cap70-lds-general-moving", 0.105, 1)),
}


def attach(P, M, columns):
    """src [P][M], scale [P][M], anchor [P][M][3] from {(p, column): (q, scale, anchor)}"""
    src = np.full((P, M), -1, dtype=np.int32)
    scale = np.ones((P, M))
    anchor = np.zeros((P, M, 3))
    for (p, i), (q, s, a) in columns.items():
        src[p, i] = q
        scale[p, i] = s
        anchor[p, i] = a
    return src, scale, anchor


SIDE = np.array([-0.25, 0.0, 0.0])


def dual_attach(M, side=SIDE):
    """the dual-arm coupling the suites run: of each arm's list, column 0 is a sphere 0.25 m beside the other arm's end
    effector -- for arm 0 about 0.5 m away at the start, outside its detection shell, which it enters mid-rollout as
    arm 1 crosses over -- and column M - 1 a point 0.8 of the way from a base to that end effector, a crude link sphere
    about 0.3 m from this arm: inside the shell throughout, so its velocity counts at every step"""
    s0 = np.array([-0.6, -0.125, 0.7])
    bases = (s0 + np.array([-0.2, -1.0, 0.0]), s0 + np.array([0.5, 1.5, 0.0]))
    cols = {}
    for p in range(2):
        cols[(p, 0)] = (1 - p, 1.0, side * (1.0 - 2.0 * p))
        cols[(p, M - 1)] = (1 - p, 0.8, 0.2 * bases[p])
    return attach(2, M, cols)
