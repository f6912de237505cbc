"""Reference of the cross audit (include/pmaf.h: pmaf_cross_audit, pmaf_cross_audit_tracks, pmaf_select_pair), written
from its stated semantics and nothing else: plain Python floats (IEEE double, round to nearest, no fused operations)
and math.sqrt (correctly rounded), one operation per line, in the order the contract gives. Test infrastructure: it
imports neither the oracle nor the package; the caller passes the library's evaluation order (pmaf_eval_order():
0 = (a0 b0 + a1 b1) + a2 b2, 1 = a0 b0 + (a1 b1 + a2 b2)). Every case is decidable, so callers compare every output at
tolerance 0."""
import math

INF = float("inf")
NAN = float("nan")


def squared_distance(x, y, right_assoc):
    """d2 = dot(x - y, x - y) in the given association"""
    dx = x[0] - y[0]
    dy = x[1] - y[1]
    dz = x[2] - y[2]
    xx = dx * dx
    yy = dy * dy
    zz = dz * dz
    if right_assoc:
        t = yy + zz
        s = xx + t
    else:
        t = xx + yy
        s = t + zz
    return s


def pair_clearance(path_a, path_b, separation, right_assoc):
    """path_a: the n points of one path of set A, path_b: the m points of one path of set B, on one step grid.
    Returns (clearance, step)."""
    n = len(path_a)
    m = len(path_b)
    if n == 0 or m == 0:
        return INF, -1
    pa = [(float(p[0]), float(p[1]), float(p[2])) for p in path_a]
    pb = [(float(p[0]), float(p[1]), float(p[2])) for p in path_b]
    big_k = max(n, m)
    best = INF
    step = -1
    for k in range(big_k):
        x = pa[min(k, n - 1)]      # hold: an ended path stays at its last point
        y = pb[min(k, m - 1)]
        d2 = squared_distance(x, y, right_assoc)
        if d2 < best:              # strict, k ascending: ties keep the smallest k; NaN never wins
            best = d2
            step = k
    if step < 0:
        return INF, -1
    root = math.sqrt(best)         # best is >= 0 or +inf here (it won a `<` against +inf or a smaller value)
    clearance = root - float(separation)
    return clearance, step


def cross_audit(paths_a, n_a, paths_b, n_b, separation, right_assoc):
    """paths_a [Na][cap][3] with n_a [Na] points each, paths_b [Nb][cap][3] with n_b [Nb] (anything indexable).
    Returns (clearance, step), nested lists [Na][Nb]."""
    a = [[paths_a[i][k] for k in range(int(n_a[i]))] for i in range(len(n_a))]
    b = [[paths_b[j][k] for k in range(int(n_b[j]))] for j in range(len(n_b))]
    clearance = []
    step = []
    for pa in a:
        crow = []
        srow = []
        for pb in b:
            c, s = pair_clearance(pa, pb, separation, right_assoc)
            crow.append(c)
            srow.append(s)
        clearance.append(crow)
        step.append(srow)
    return clearance, step


def select_pair(clearance, cost_a, cost_b, margin):
    """clearance [Na][Nb], cost_a [Na], cost_b [Nb]. Returns (pair, pair_cost, pair_clearance, feasible)."""
    margin = float(margin)
    best_sum = INF
    pair = (-1, -1)
    for i in range(len(cost_a)):
        for j in range(len(cost_b)):
            c = float(clearance[i][j])
            if not c >= margin:    # infeasible; a NaN clearance is
                continue
            s = float(cost_a[i]) + float(cost_b[j])
            if s < best_sum:       # strict, row-major: ties keep the smallest i, then the smallest j; NaN never wins
                best_sum = s
                pair = (i, j)
    if pair != (-1, -1):
        return pair, best_sum, float(clearance[pair[0]][pair[1]]), 1
    best_clr = -INF
    for i in range(len(cost_a)):
        for j in range(len(cost_b)):
            c = float(clearance[i][j])
            if c > best_clr:
                best_clr = c
                pair = (i, j)
    if pair == (-1, -1):
        return pair, NAN, NAN, 0
    s = float(cost_a[pair[0]]) + float(cost_b[pair[1]])
    return pair, s, best_clr, 0
