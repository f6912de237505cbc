"""The joint selection's cases (pmaf_select_pair_clear / pmaf_select_clear_tracks), shared by tests/test_pair_clear.py
(CPU: the oracle's rollouts, where the margins below are chosen and shown to reach every rule) and
tests/test_pair_clear_gpu.py (the same scenes and the same parametrisation on the device). Test infrastructure: scene
construction and the parameter lists only; it imports neither the package nor the oracle."""
import numpy as np

SEP = 0.15          # radius 0.05 + DualArmCoupling's self-collision radius 0.1
RADIUS = 0.05

# (P, N, M, H, ragged, (pop_a, pop_b)) and what each reaches:
#   (2, 5, 2, 8)       the base case
#   (2, 5, 66, 70)     a second obstacle tile, several chunks of 16 steps, a skipped trailing obstacle in the second tile
#   (2, 5, 2, 70) ragged   windows shorter than paths and paths shorter than windows: the hold rule is reached
#   (2, 33, 2, 8)      the 32-path tile edge on both axes
#   (2, 65, 2, 8)      4 225 pairs: several reduction blocks and the second stage
#   (3, 5, 2, 8) (2, 0)    population offsets with a > b
SHAPES = [(2, 5, 2, 8, False, (0, 1)), (2, 5, 66, 70, False, (0, 1)), (2, 5, 2, 70, True, (0, 1)),
          (2, 33, 2, 8, False, (0, 1)), (2, 65, 2, 8, False, (0, 1)), (3, 5, 2, 8, False, (2, 0))]
SLACK_SHAPES = [SHAPES[1], SHAPES[2]]      # the two N = 5 shapes that have enough steps


def shape_id(s):
    return "P%d-N%d-M%d-H%d%s-a%db%d" % (s[0], s[1], s[2], s[3], "-ragged" if s[4] else "", s[5][0], s[5][1])


def horizons(H):
    return (1, 3, H // 2, H + 1, H + 6)


def lates(cap):
    return (None, (0, 0), (2, 0), (1, 3), (cap, cap))


def build_scenes(scenes, P, N, M, H, ragged):
    """P differing synthetic scenes, every obstacle moving, different gains per agent (different paths and costs). The
    arms start 0.2 m apart in y and their goals are swapped in y, so the paths close in on each other along the horizon
    and the window matters to the pair side. The trailing obstacle of every arm is a sphere beside its first path
    points, as the coupled configuration's set-point sphere is. The ragged case is test_path_audit_gpu.rollout_case's."""
    scs = []
    for p in range(P):
        sc = scenes.synthetic_scene(N, H, M, config_id=7, scene_id=p, dynamic=True)
        if ragged:   # close to the goal, agents of different stiffness: some rollouts end at the goal guard, some do not
            sc["start"] = sc["goal"] - np.array([0.13, 0.01 * p, 0.0])
            sc["k_attr"] = np.linspace(1.0, 8.0, N)
        else:
            sc["k_attr"] = np.linspace(2.0, 6.0, N)
            sc["k_circ"] = np.linspace(0.02, 0.04, N)
            sc["k_damp"] = np.linspace(2.5, 4.0, N)
            sc["start"] = sc["start"] + np.array([0.0, 0.2 * p, 0.0])
            sc["goal"] = sc["goal"] + np.array([0.0, 0.1 - 0.2 * p, 0.0])
        if ragged:
            sc["obstacles"][-1] = [0.05 * p, 0.2, 0.8, -0.04, 0.03 + 0.01 * p, -0.02, 0.1]
        else:
            side = -1.0 if p % 2 == 0 else 1.0      # on the arm's outer side
            at = sc["start"] + np.array([0.04, 0.155 * side, 0.0])
            sc["obstacles"][-1] = [at[0], at[1], at[2], -0.04, -0.03 * side, -0.02, 0.1]
        scs.append(sc)
    return scs


def live_list(scenes, start):
    """the tick's fresh list: the start list one node period later, the trailing obstacle moved as well"""
    live = np.stack([scenes.advance_live_obstacles(o) for o in start])
    live[:, -1, 0:3] += np.array([0.01, -0.02, 0.005])
    return live


def previous_pairs(N, k):
    """the previous pair handed to the k-th call of a shape: every other call has none"""
    if k % 2 == 0:
        return None
    return ((3 * k) % N, (5 * k + 1) % N)


# (obstacle_margin, pair_margin), chosen on the oracle's rollouts of the scenes above (tests/test_pair_clear.py asserts what
# they reach). Every shape: everything feasible / nobody clear / no pair apart. Then per shape values that cut through
# its clearances at some horizon:
#   H = 8 shapes       every agent of an arm has the same first points: c = 0.0321 / -0.0060 with the trailing sphere,
#                      0.13 .. 0.53 without it; the pair clearance is 0.05 at horizon 1 and 0.04496 from horizon 3 on
#   (2, 5, 66, 70)     without the trailing sphere c_b = 0.10826 .. 0.10832 from horizon 35 on; the pair clearances are
#                      -0.12074 .. -0.12035 at horizon 35 and -0.14848 .. -0.14713 at the full horizon
#   ragged             c_b = 0.14502 .. 0.1588, pair clearances -0.141 .. -0.14 at the full horizon
EVERY_SHAPE = [(-0.5, -0.5), (3.0, -0.5), (-0.5, 3.0)]
MARGINS = {
    8: EVERY_SHAPE + [(0.01, 0.0449), (-0.5, 0.0449)],
    (70, False): EVERY_SHAPE + [(0.10827, -0.1477), (0.10827, -0.1206), (-0.5, -0.1477)],
    (70, True): EVERY_SHAPE + [(0.157, -0.1405), (0.157, -0.5), (-0.5, -0.1405)],
}


def margins(shape):
    H, ragged = shape[3], shape[4]
    return MARGINS[8] if H == 8 else MARGINS[(H, ragged)]


def calls(shape):
    """the parametrisation of one shape: dicts of horizon, obstacle_margin, pair_margin, skip_trailing, late, prev_pair"""
    P, N, M, H, ragged, _ = shape
    out = []
    k = 0
    for horizon in horizons(H):
        for om, pm in margins(shape):
            for skip in (0, 1):
                for _ in range(2):        # without and with a previous pair
                    out.append(dict(horizon=horizon, obstacle_margin=om, pair_margin=pm, skip_trailing=skip, late=None,
                                    prev_pair=previous_pairs(N, k)))
                    k += 1
    if shape in SLACK_SHAPES:
        for late in lates(H + 1)[1:]:
            for horizon in (3, H // 2, H + 1):
                for om, pm in margins(shape)[3:]:
                    out.append(dict(horizon=horizon, obstacle_margin=om, pair_margin=pm, skip_trailing=1, late=late,
                                    prev_pair=previous_pairs(N, k)))
                    k += 1
    return out
