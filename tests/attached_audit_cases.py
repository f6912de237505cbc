"""The cases of the joint selection on coupled handles (pmaf_cross_audit_attached / pmaf_select_pair_clear_tracked),
shared by tests/test_attached_audit.py (CPU: the oracle's rollouts, where the cases are shown to be sensitive and the
GPU cases' pre-conditions are asserted) and tests/test_attached_audit_gpu.py (the same scenes on the device). Test
infrastructure: scene construction and the couplings only; it imports neither the package nor the oracle."""
import numpy as np

SEP = 0.15          # radius 0.05 + DualArmCoupling's self-collision radius 0.1
T = 32              # csrc/pmaf_cross_audit.hpp's tile edge (the GPU suite reads the header and asserts this value)

# name -> P, N, M, cap, general (mass != 1 and an agent with k_attr == 0: the general step), ragged (arm 1's goal is
# 0.13 m from its start and its agents differ in stiffness: paths of different lengths, the hold rule acts).
#   cap 9: below one chunk of 16 steps; cap 70: four chunks and a ragged fifth
#   N = 5: one ragged tile; N = T + 1: a ragged second tile on both axes
SHAPES = {
    "P2-N5-M3-cap9": dict(P=2, N=5, M=3, cap=9, general=False, ragged=False),
    "P2-N5-M3-cap70-ragged": dict(P=2, N=5, M=3, cap=70, general=False, ragged=True),
    "P2-N33-M3-cap70-ragged": dict(P=2, N=T + 1, M=3, cap=70, general=False, ragged=True),
    "P2-N5-M60-cap70-general-ragged": dict(P=2, N=5, M=60, cap=70, general=True, ragged=True),
    "P3-N5-M3-cap70-ragged": dict(P=3, N=5, M=3, cap=70, general=False, ragged=True),
}
# the shape groups of the rollout kernels the coupled handles run (tests/sentinel_track_reference.py)
SHAPE_GROUPS = {
    "plain": ("P2-N5-M3-cap9", "P2-N5-M3-cap70-ragged", "P3-N5-M3-cap70-ragged"),
    "general": ("P2-N5-M60-cap70-general-ragged",),
}
# attachment kinds per shape: every shape runs none / one / tie / three; the M = 60 shape also all of one side
KINDS = ("none", "one", "tie", "three")


def kinds(shape):
    return KINDS + (("all",) if SHAPES[shape]["M"] == 60 else ())


def build_scenes(scenes, shape):
    """P arms of one handle on the one-slot wave-per-agent route (M <= 60): arm 1 starts 0.3 m in front of and 0.5 m
    beside arm 0 and travels ACROSS its front (tests/field_couple_reference.dual_scenes' geometry), so what rides on one
    arm's path moves relative to the other arm; a third arm on the other side with a goal 0.13 m away. Every field
    obstacle is at rest but one; the trailing sphere rests at another arm's start."""
    s = SHAPES[shape]
    N = s["N"]
    scs = []
    for p in range(s["P"]):
        sc = scenes.synthetic_scene(N, s["cap"] - 1, s["M"], config_id=11, scene_id=p, dynamic=False)
        sc["obstacles"][1, 3:6] = [0.04, -0.03, 0.02]
        sc["k_attr"] = np.linspace(3.0, 5.0, N)
        sc["k_repel"] = np.linspace(0.06, 0.1, N)
        if p == 0:
            sc["k_damp"] = np.linspace(2.0, 4.0, N)
        scs.append(sc)
    s0 = np.array(scs[0]["start"], dtype=np.float64)
    scs[1]["start"] = s0 + np.array([0.3, 0.5, 0.0])
    scs[1]["goal"] = scs[1]["start"] + np.array([0.0, -0.13 if s["ragged"] else -1.2, 0.0])
    if s["ragged"]:
        scs[1]["k_attr"] = np.linspace(1.0, 8.0, N)
    if s["P"] > 2:
        scs[2]["start"] = s0 + np.array([0.3, -0.5, 0.0])
        scs[2]["goal"] = scs[2]["start"] + np.array([0.0, 0.13, 0.0])
    if s["general"]:
        for sc in scs:
            sc["agent_mass"] = 1.25
            sc["k_attr"][2] = 0.0
    for p in range(s["P"]):
        q = (p + 1) % 2 if p < 2 else 0
        scs[p]["obstacles"][-1] = list(scs[q]["start"]) + [0.0, 0.0, 0.0, 0.1]
    return scs


def coupling(shape, kind, scs, shift=1):
    """dict(src [P][M], scale [P][M], anchor [P][M][3], shift) of one attachment kind between populations 0 and 1, or
    None for `none`.
      one     column 0 of arm 0's list is a sphere about 0.25 m beside arm 1's end effector (scale 0.9)
      tie     column 0 of both lists is the other end effector itself (scale 1, anchor 0): d2 ties with term 0, and at a
              separation of radius + r the gap ties as well
      three   per side columns 0, 1, 2: the other end effector itself (scale 1, anchor 0: d2 ties with term 0 at another
              R), a sphere at rest (scale 0) 0.2 m in front of this arm's start, and a point 0.8 of the way from a base
              to the other end effector, a crude link sphere -- different scales and anchors on the two sides
      all     every column of arm 0's list rides on arm 1 (M = 60), scales 0.5 .. 1.09, anchors spread over 0.4 m
    In a handle of three populations, column 2 of arm 0's list rides on population 2 in every kind but `none`: it is not
    a term of the pair (0, 1) and stays on the obstacle side."""
    s = SHAPES[shape]
    P, M = s["P"], s["M"]
    if kind == "none":
        return None
    src = np.full((P, M), -1, dtype=np.int32)
    scale = np.ones((P, M))
    anchor = np.zeros((P, M, 3))
    starts = [np.array(sc["start"], dtype=np.float64) for sc in scs]
    if kind == "one":
        src[0, 0] = 1
        scale[0, 0] = 0.9
        anchor[0, 0] = 0.1 * starts[1] + np.array([-0.25, 0.0, 0.0])
    elif kind == "tie":
        src[0, 0], src[1, 0] = 1, 0
    elif kind == "three":
        bases = (starts[0] + np.array([-0.2, -1.0, 0.0]), starts[0] + np.array([0.5, 1.5, 0.0]))
        for p in (0, 1):
            src[p, 0:3] = 1 - p
            scale[p, 1] = 0.0
            anchor[p, 1] = starts[p] + np.array([0.2, 0.02 * (1 - 2 * p), 0.01])
            scale[p, 2] = 0.8 - 0.1 * p
            anchor[p, 2] = (0.2 + 0.1 * p) * bases[p]
    elif kind == "all":
        src[0, :] = 1
        scale[0, :] = 0.5 + 0.01 * np.arange(M)
        anchor[0, :, 0] = 0.4 * np.cos(np.arange(M))
        anchor[0, :, 1] = 0.4 * np.sin(0.7 * np.arange(M))
        anchor[0, :, 2] = 0.02 * np.arange(M) / M
    else:
        raise ValueError(kind)
    if P > 2:
        src[0, 2] = 2
        scale[0, 2] = 1.0
        anchor[0, 2] = [0.0, 0.3, 0.0]
    return dict(src=src, scale=scale, anchor=anchor, shift=shift)


def live_list(scenes, scs):
    """the tick's fresh list [P][n_obs][7]: the creation lists one node period later, every radius 1.1 times the creation
    list's (the attached terms and the obstacle side read the CALLER'S radii), the trailing sphere moved as well"""
    live = np.stack([scenes.advance_live_obstacles(np.array(sc["obstacles"], dtype=np.float64)) for sc in scs])
    live[:, :, 6] *= 1.1
    live[:, -1, 0:3] += np.array([0.01, -0.02, 0.005])
    return live


def sphere_on_the_pair(P, M, paths, n, pair, k, side, column=0, shift=0):
    """the coupling of the behavioural case: one column of A's list (side 0) or of B's (side 1) with scale 1 and
    anchor = x_i(k) - y_j(k) (or its negation), so the sphere riding on the pair's other member sits on this member's
    point at step k. paths [P][N][cap][3], n [P][N], pair (i, j) of populations 0 and 1."""
    i, j = pair
    x = np.array(paths[0][i][min(k, int(n[0][i]) - 1)], dtype=np.float64)
    y = np.array(paths[1][j][min(k, int(n[1][j]) - 1)], dtype=np.float64)
    src = np.full((P, M), -1, dtype=np.int32)
    scale = np.ones((P, M))
    anchor = np.zeros((P, M, 3))
    src[side, column] = 1 - side
    anchor[side, column] = (x - y) if side == 0 else (y - x)
    return dict(src=src, scale=scale, anchor=anchor, shift=shift)


def far_rows(live, cpl):
    """the live list with the attached columns' rows far away (30 m up, at rest): the untracked calls do not see them"""
    out = np.array(live, dtype=np.float64, copy=True)
    P, M = cpl["src"].shape
    for p in range(P):
        for s in range(M):
            if cpl["src"][p][s] >= 0:
                out[p, s, 0:6] = [0.0, 0.0, 30.0, 0.0, 0.0, 0.0]
    return out
