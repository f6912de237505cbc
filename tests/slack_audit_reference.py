"""Reference of the cross audit with timing slack (include/pmaf.h: pmaf_cross_audit_slack, pmaf_cross_audit_tracks_slack,
pmaf_select_pair_slack), written from its stated semantics and nothing else: plain Python floats (IEEE double, round to
nearest, no fused operations) and math.sqrt (correctly rounded), a literal double loop over k, then l, with a strict `<`.
Test infrastructure: it imports neither the oracle nor the package, only the cross audit reference's squared distance;
the caller passes the library's evaluation order (pmaf_eval_order()). Every case is decidable, so callers compare every
output at tolerance 0. The pair rule on the slacked matrix is cross_audit_reference.select_pair, unchanged."""
import math

from cross_audit_reference import squared_distance

INF = float("inf")


def _points(path):
    return [(float(p[0]), float(p[1]), float(p[2])) for p in path]


def pair_clearance_slack(path_a, path_b, separation, late_a, late_b, right_assoc):
    """path_a: the n points of one path of set A, path_b: the m points of one path of set B, on one step grid; A may be
    up to late_a steps behind B's clock, B up to late_b behind A's. Returns (clearance, step_a, step_b)."""
    late_a = int(late_a)
    late_b = int(late_b)
    assert late_a >= 0 and late_b >= 0
    n = len(path_a)
    m = len(path_b)
    if n == 0 or m == 0:
        return INF, -1, -1
    pa = _points(path_a)
    pb = _points(path_b)
    big_k = max(n, m)
    best = INF
    step_a = -1
    step_b = -1
    for k in range(big_k):
        x = pa[min(k, n - 1)]          # hold: an ended path stays at its last point
        first = max(0, k - late_b)     # admitted: -late_b <= l - k <= late_a, 0 <= l < K
        last = min(big_k - 1, k + late_a)
        for l in range(first, last + 1):
            y = pb[min(l, m - 1)]
            d2 = squared_distance(x, y, right_assoc)
            if d2 < best:              # strict, k then l ascending: ties keep the smallest (k, l); NaN never wins
                best = d2
                step_a = k
                step_b = l
    if step_a < 0:
        return INF, -1, -1
    root = math.sqrt(best)
    clearance = root - float(separation)
    return clearance, step_a, step_b


def cross_audit_slack(paths_a, n_a, paths_b, n_b, separation, late_a, late_b, right_assoc):
    """paths_a [Na][cap][3] with n_a [Na] points each, paths_b [Nb][cap][3] with n_b [Nb] (anything indexable).
    Returns (clearance, step_a, step_b), nested lists [Na][Nb]."""
    a = [_points([paths_a[i][k] for k in range(int(n_a[i]))]) for i in range(len(n_a))]
    b = [_points([paths_b[j][k] for k in range(int(n_b[j]))]) for j in range(len(n_b))]
    clearance = []
    step_a = []
    step_b = []
    for pa in a:
        crow = []
        arow = []
        brow = []
        for pb in b:
            c, sa, sb = pair_clearance_slack(pa, pb, separation, late_a, late_b, right_assoc)
            crow.append(c)
            arow.append(sa)
            brow.append(sb)
        clearance.append(crow)
        step_a.append(arow)
        step_b.append(brow)
    return clearance, step_a, step_b
