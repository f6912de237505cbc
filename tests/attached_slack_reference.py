"""Reference of the joint selection on coupled handles with timing slack (include/pmaf.h:
pmaf_cross_audit_attached_slack, pmaf_select_pair_clear_tracked_slack), written from their stated contract and nothing
else. Plain Python floats. Test infrastructure: it imports neither the oracle nor the package. Every case is decidable,
so callers compare every output at tolerance 0.

It is a composition. The term rule -- which spheres a pair is held to, where they ride, their radii -- is
attached_audit_reference.terms_of / ride. The ride is per point, so a slacked term is the slacked audit
(slack_audit_reference.pair_clearance_slack, with R in the place of the separation) of path_a against the ridden path_b
(a term 1 + s: the sphere is on B's clock) or of the ridden path_a against path_b (a term 1 + M + s). In the second case
the audit's d is z - yh_l, the negation of the contract's u - z: every component's square has the same bits. The hold
rule needs no word of its own: the ride of a held point is the held ride. The fold goes in term order with a strict `<`.
The joint call is composed around pair_clear_reference.select_pair_clear as attached_audit_reference composes its own.

MUTANTS name the ways an implementation can misread the contract; tests/test_attached_slack_audit.py shows that each of
them changes an output in every shape group the GPU suite runs."""
import math

import attached_audit_reference as aar
import pair_clear_reference as pcr
import select_clear_reference as scr
import slack_audit_reference as sar
from cross_audit_reference import squared_distance

INF = float("inf")
#   spheres_unslacked  the slack applied to term 0 only, the spheres step against step: the limit this call lifts
#   late_swapped       late_a / late_b swapped on the sphere terms
#   wrong_clock        the sphere of a term 1 + s taken at k instead of l
#   band               a band off by one (l - k <= late_a + 1)
#   tie_lk             ties inside a term go to the least (l, k) instead of the least (k, l)
#   late_term          ties between terms go to the later term
#   nohold             K = min(n, m): no hold
#   separation         R = separation for every term
MUTANTS = ("spheres_unslacked", "late_swapped", "wrong_clock", "band", "tie_lk", "late_term", "nohold", "separation")


def _scan(pa, pb, R, late_a, late_b, right_assoc, mutant, z_at_k=None):
    """the mutants' own scan of one term (the contract's scan is slack_audit_reference's): pa, pb the staged paths.
    z_at_k: wrong_clock -- B's side is read at k whatever l is."""
    n, m = len(pa), len(pb)
    big_k = min(n, m) if mutant == "nohold" else max(n, m)
    up = late_a + (1 if mutant == "band" else 0)
    best, sa, sb = INF, -1, -1
    if mutant == "tie_lk":
        for l in range(big_k):
            y = pb[min(l, m - 1)]
            for k in range(max(0, l - up), min(big_k - 1, l + late_b) + 1):
                d2 = squared_distance(pa[min(k, n - 1)], y, right_assoc)
                if d2 < best:
                    best, sa, sb = d2, k, l
    else:
        for k in range(big_k):
            x = pa[min(k, n - 1)]
            for l in range(max(0, k - late_b), min(big_k - 1, k + up) + 1):
                y = pb[min(k if z_at_k else l, m - 1)]
                d2 = squared_distance(x, y, right_assoc)
                if d2 < best:
                    best, sa, sb = d2, k, l
    if sa < 0:
        return INF, -1, -1
    return math.sqrt(best) - float(R), sa, sb


def attached_slack_pair(path_a, path_b, terms, late_a, late_b, right_assoc, mutant=None):
    """path_a: the n points of one path of set A, path_b: the m points of one of set B; terms:
    attached_audit_reference.terms_of's. Returns (clearance, step_a, step_b, sphere)."""
    late_a, late_b = int(late_a), int(late_b)
    assert late_a >= 0 and late_b >= 0
    if len(path_a) == 0 or len(path_b) == 0:
        return INF, -1, -1, -1
    pa = [tuple(float(c) for c in p) for p in path_a]
    pb = [tuple(float(c) for c in p) for p in path_b]
    best = (INF, -1, -1, -1)
    for code, on_b, scale, anchor, R in terms:
        la, lb = late_a, late_b
        if code == 0:
            sa_path, sb_path = pa, pb
        else:
            if mutant == "spheres_unslacked":
                la, lb = 0, 0
            if mutant == "late_swapped":
                la, lb = late_b, late_a
            if on_b:    # a sphere of A's list that rides on arm B: on B's clock
                sa_path, sb_path = pa, [tuple(aar.ride(p, scale, anchor)) for p in pb]
            else:       # a sphere of B's list that rides on arm A: on A's clock
                sa_path, sb_path = [tuple(aar.ride(p, scale, anchor)) for p in pa], pb
        if mutant in ("band", "tie_lk", "nohold") or (mutant == "wrong_clock" and code != 0 and on_b):
            gap, k, l = _scan(sa_path, sb_path, R, la, lb, right_assoc, mutant, mutant == "wrong_clock")
        else:
            gap, k, l = sar.pair_clearance_slack(sa_path, sb_path, R, la, lb, right_assoc)
        if k < 0:
            continue                                # nothing won the term (every d2 NaN): gap = +inf, never folded
        take = gap < best[0]                        # strict, terms ascending: ties keep the smallest term
        if mutant == "late_term":
            take = gap <= best[0]
        if take:
            best = (gap, k, l, code)
    return best


def cross_audit_attached_slack(paths_a, n_a, paths_b, n_b, coupling, pop_a, pop_b, obstacles, rad, separation, late_a, late_b,
                               right_assoc, mutant=None):
    """paths_a [Na][cap][3] with n_a [Na] points each, paths_b alike. Returns (clearance, step_a, step_b, sphere), nested
    lists [Na][Nb]."""
    terms = aar.terms_of(coupling, pop_a, pop_b, obstacles, rad, separation, "separation" if mutant == "separation" else None)
    a = [[paths_a[i][k] for k in range(int(n_a[i]))] for i in range(len(n_a))]
    b = [[paths_b[j][k] for k in range(int(n_b[j]))] for j in range(len(n_b))]
    out = ([], [], [], [])
    for pa in a:
        rows = ([], [], [], [])
        for pb in b:
            r = attached_slack_pair(pa, pb, terms, late_a, late_b, right_assoc, mutant)
            for dst, v in zip(rows, r):
                dst.append(v)
        for dst, row in zip(out, rows):
            dst.append(row)
    return out


def pair_side(paths_a, n_a, paths_b, n_b, coupling, pop_a, pop_b, obstacles, rad, horizon, separation, late, right_assoc,
              mutant=None):
    """(clearance, step_a, step_b, w_a, w_b): the slacked attached audit on the two path sets cut to w = min(n, horizon)
    points -- pair_clear_reference.pair_side's tuple. late = (late_a, late_b)."""
    w_a = scr.windows([n_a], horizon)[0]
    w_b = scr.windows([n_b], horizon)[0]
    clearance, step_a, step_b, _ = cross_audit_attached_slack(paths_a, w_a, paths_b, w_b, coupling, pop_a, pop_b, obstacles, rad,
                                                              separation, late[0], late[1], right_assoc, mutant)
    return clearance, step_a, step_b, w_a, w_b


def select_pair_clear_tracked_slack(paths, n_points, obstacles, tracks, first, coupling, costs, dt, rad, pop_a, pop_b,
                                    obstacle_margin, horizon, skip_trailing, separation, pair_margin, late, prev_pair,
                                    right_assoc, audited=None, matrix=None, mutant=None):
    """pmaf_select_pair_clear_tracked_slack: pair_clear_reference.select_pair_clear's dict. late = None is
    attached_audit_reference.select_pair_clear_tracked. audited / matrix: what attached_audit_reference.obstacle_side /
    pair_side above returned for the same inputs (computed once, shared, never modified)."""
    if late is None:
        return aar.select_pair_clear_tracked(paths, n_points, obstacles, tracks, first, coupling, costs, dt, rad, pop_a, pop_b,
                                             obstacle_margin, horizon, skip_trailing, separation, pair_margin, prev_pair,
                                             right_assoc, audited, matrix)
    if audited is None:     # the obstacle side is unchanged
        audited = aar.obstacle_side(paths, n_points, obstacles, tracks, first, coupling, pop_a, pop_b, dt, rad, obstacle_margin,
                                    horizon, skip_trailing, right_assoc)
    if matrix is None:
        matrix = pair_side(paths[pop_a], n_points[pop_a], paths[pop_b], n_points[pop_b], coupling, pop_a, pop_b, obstacles, rad,
                           horizon, separation, late, right_assoc, mutant)
    return pcr.select_pair_clear(paths, n_points, obstacles, costs, dt, rad, pop_a, pop_b, obstacle_margin, horizon,
                                 skip_trailing, separation, pair_margin, late, prev_pair, right_assoc, audited, matrix)
