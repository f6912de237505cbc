"""The cases of the joint selection on coupled handles with timing slack (pmaf_cross_audit_attached_slack /
pmaf_select_pair_clear_tracked_slack), shared by tests/test_attached_slack_audit.py (CPU: the oracle's rollouts) and
tests/test_attached_slack_audit_gpu.py (the same scenes on the device). Shapes, attachment kinds, couplings and the live
list are tests/attached_audit_cases.py's, by import; this file adds the slacks and ONE shape for the behavioural case.
Test infrastructure: it imports neither the package nor the oracle.

Why a shape of its own: at dt = 0.01 an agent moves about 1 mm per step against R >= 0.05, so in the existing shapes no
collision exists that ONLY a slack of a few steps reveals. At dt = 0.1 the arms move centimetres per step."""
import numpy as np

import attached_audit_cases as aac

SEP = aac.SEP
T = aac.T
C = 16              # csrc/pmaf_cross_audit.hpp's chunk of steps (the GPU suite reads the header and asserts this value)
SHAPES = aac.SHAPES
SHAPE_GROUPS = aac.SHAPE_GROUPS
kinds = aac.kinds
coupling = aac.coupling
live_list = aac.live_list

# the behavioural shape: build_scenes' geometry of P = 2, N = 5, M = 3, not ragged, with 24 points per path and dt = 0.1
LATE_SHAPE = "P2-N5-M3-cap24-dt0.1"
LATE_CAP = 24
LATE_D = 5          # the lag of the behavioural case, in steps
LATE_RADIUS = 0.01  # the caller's radius of the attached column


def slacks(cap):
    """the slack list of a capacity: the diagonal, one step either way, a small asymmetric band, (C - 1, C) -- the
    diagonal chunk pair just outside the band on either side --, bands wider than one and two chunks on one side only,
    everything, and far beyond everything (clamped on the host: equal to `cap`)"""
    return [(0, 0), (1, 0), (0, 1), (3, 2), (C - 1, C), (C + 1, 0), (0, 2 * C + 3), (cap, cap), (10 ** 6, 10 ** 6)]


def chain(cap):
    """slacks along which the clearance may only fall"""
    return [(0, 0), (1, 0), (3, 2), (C - 1, C), (cap, cap)]


def build_scenes(scenes, shape):
    if shape != LATE_SHAPE:
        return aac.build_scenes(scenes, shape)
    scs = aac.build_scenes(scenes, "P2-N5-M3-cap9")     # (the capacity enters a scene as max_prediction_steps only)
    for sc in scs:
        sc["max_prediction_steps"] = LATE_CAP
        sc["dt"] = 0.1
    return scs


def shape_of(shape):
    if shape == LATE_SHAPE:
        return dict(P=2, N=5, M=3, cap=LATE_CAP, general=False, ragged=False)
    return SHAPES[shape]


def late_step(n, d=LATE_D):
    """the step of the behavioural case: as deep as both populations' shortest paths go with d steps to spare"""
    return min(int(v) for row in n for v in row) - 1 - d


def sphere_on_the_late_pair(P, M, paths, n, pair, k, d, side):
    """the coupling of the behavioural case: column 0 of one list on the other member of the pair, scale 1.
      side 0  column 0 of A's list rides on B's candidate, anchor = x_i(k) - y_j(k + d): the sphere at B's step k + d
              sits on A's point at step k. It is hit iff A may run d steps behind B's clock: late_a >= d.
      side 1  the mirror image: column 0 of B's list rides on A's candidate, anchor = -(x_i(k + d) - y_j(k)): the sphere
              at A's step k + d sits on B's point at step k. It is hit iff late_b >= d.
    paths [P][N][cap][3], n [P][N], pair (i, j) of populations 0 and 1."""
    i, j = pair
    ka, kb = (k, k + d) if side == 0 else (k + d, k)
    x = np.array(paths[0][i][min(ka, int(n[0][i]) - 1)], dtype=np.float64)
    y = np.array(paths[1][j][min(kb, int(n[1][j]) - 1)], dtype=np.float64)
    src = np.full((P, M), -1, dtype=np.int32)
    scale = np.ones((P, M))
    anchor = np.zeros((P, M, 3))
    src[side, 0] = 1 - side
    anchor[side, 0] = (x - y) if side == 0 else -(x - y)
    return dict(src=src, scale=scale, anchor=anchor, shift=0)


def late_slack(side, d=LATE_D, wrong=False):
    """the slack that reveals the behavioural case's collision, or the same lag the wrong way round"""
    hit = (d, 0) if side == 0 else (0, d)
    return (hit[1], hit[0]) if wrong else hit


def late_rows(live, cpl):
    """the live list with the attached columns' rows far away (far_rows) and their radius -- the caller's, which the
    terms read -- set to LATE_RADIUS"""
    out = aac.far_rows(live, cpl)
    P, M = cpl["src"].shape
    for p in range(P):
        for s in range(M):
            if cpl["src"][p][s] >= 0:
                out[p, s, 6] = LATE_RADIUS
    return out


TWIN_SEP = 0.01     # below every sphere's R: in a twin pair (i, i) term 0 is 0 m apart on the diagonal


def twin_coupling(P, M, paths, n, agent, gap=2):
    """a tie INSIDE a term, which rollouts of two different arms never give. Where both populations have the same paths
    (twin scenes), column 0 of A's list with scale -1 and anchor a = RN(x(ka) + x(kb)) of one agent puts the sphere at
    z_l = RN(a - x_l). With e = a - (x(ka) + x(kb)) the rounding error of the anchor, u - z is -e at (ka, kb) AND at
    (kb, ka) wherever both differences a - x are exact: the minimum of the pair (agent, agent), some 1e-17 m, is attained
    twice, and the order (d2, k, l) decides which steps are reported. Returns (coupling, ka, kb): the first ka >= 1 with
    kb = ka + gap at which the two vectors are equal in every component."""
    x = np.array(paths[0][agent], dtype=np.float64)[:int(n[0][agent])]
    for ka in range(1, len(x) - gap):
        kb = ka + gap
        a = x[ka] + x[kb]
        if ((x[ka] - (a - x[kb])) == (x[kb] - (a - x[ka]))).all():
            src = np.full((P, M), -1, dtype=np.int32)
            scale = np.ones((P, M))
            anchor = np.zeros((P, M, 3))
            src[0, 0] = 1
            scale[0, 0] = -1.0
            anchor[0, 0] = a
            return dict(src=src, scale=scale, anchor=anchor, shift=0), ka, kb
    raise AssertionError("no step of the path gives an exact tie")
