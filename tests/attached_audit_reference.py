"""Reference of the joint selection on coupled handles (include/pmaf.h: pmaf_cross_audit_attached,
pmaf_select_pair_clear_tracked), written from their stated contract and nothing else. Plain Python floats. The term rule
-- which spheres a pair is held to, where they are, their radii, the order of the minima -- is stated here directly;
everything else is composed from existing references: cross_audit_reference (the hold rule, d2, the root of term 0),
tracked_audit_reference (the obstacle side on the tracks the rollouts followed) and pair_clear_reference.joint_rule (the
rules -1 / 0 / 1 / 2). Test infrastructure: it imports neither the oracle nor the package. Every case is decidable, so
callers compare every output at tolerance 0.

A coupling is a dict(src=[P][M], scale=[P][M], anchor=[P][M][3], shift=int) -- what pmaf_couple_obstacle_tracks last
set -- or None. `shift` is carried only so that the mutant that applies it can.

MUTANTS name the ways an implementation can misread the contract; tests/test_attached_audit.py shows that each of them
changes an output in every shape group the GPU suite runs."""
import math

import cross_audit_reference as car
import pair_clear_reference as pcr
import select_clear_reference as scr
import tracked_audit_reference as tar

INF = float("inf")
NAN = float("nan")
MUTANTS = ("ignored", "swapped", "scale", "anchor", "separation", "columns_kept", "nohold", "late_term", "unwindowed",
           "shift")


def attached_columns(coupling, p, q):
    """S_pq: the columns s < M of population p's list that ride on population q's path, ascending"""
    if coupling is None:
        return []
    return [s for s, v in enumerate(coupling["src"][p]) if int(v) == q]


def terms_of(coupling, pop_a, pop_b, obstacles, rad, separation, mutant=None):
    """the terms of a pair, in order: (code, rides_on_b, scale, anchor, R). rides_on_b: the sphere is z(yh_k), held
    against xh_k; otherwise z(xh_k) against yh_k. code = 0, 1 + s or 1 + M + s."""
    terms = [(0, True, None, None, float(separation))]
    if coupling is None or mutant == "ignored":
        return terms
    M = len(obstacles[pop_a]) - 1
    for base, p, q, on_b in ((1, pop_a, pop_b, True), (1 + M, pop_b, pop_a, False)):
        for s in attached_columns(coupling, p, q):
            r = float(obstacles[p][s][6])
            R = float(rad) + r
            if mutant == "separation":
                R = float(separation)
            scale = float(coupling["scale"][p][s])
            anchor = [float(v) for v in coupling["anchor"][p][s]]
            if mutant == "scale":
                scale = 1.0
            if mutant == "anchor":
                anchor = [0.0, 0.0, 0.0]
            side = on_b
            if mutant == "swapped":
                side = not on_b
            terms.append((base + s, side, scale, anchor, R))
    return terms


def ride(point, scale, anchor):
    """z = RN(anchor + RN(scale * y)) per component: one rounded multiply, one rounded add"""
    z = []
    for c in range(3):
        m = scale * float(point[c])
        z.append(anchor[c] + m)
    return z


def attached_pair(path_a, path_b, terms, right_assoc, mutant=None, shift=0):
    """path_a: the n points of one path of set A, path_b: the m points of one of set B. Returns (clearance, step,
    sphere)."""
    n = len(path_a)
    m = len(path_b)
    if n == 0 or m == 0:
        return INF, -1, -1
    big_k = max(n, m)
    if mutant == "nohold":
        big_k = min(n, m)
    best_gap = INF
    best_step = -1
    best_code = -1
    for code, on_b, scale, anchor, R in terms:
        d2 = INF
        step = -1
        for k in range(big_k):
            x = path_a[min(k, n - 1)]          # hold: an ended path stays at its last point
            y = path_b[min(k, m - 1)]
            if code == 0:
                u, z = x, y
            else:
                src, held = (y, x) if on_b else (x, y)
                if mutant == "shift":           # (the composer's source path starts at point `shift`; the audit's does not)
                    pts, cnt = (path_b, m) if on_b else (path_a, n)
                    src = pts[min(k + shift, cnt - 1)]
                u, z = held, ride(src, scale, anchor)
            v = car.squared_distance([float(c) for c in u], [float(c) for c in z], right_assoc)
            if v < d2:                          # strict, k ascending: ties keep the smallest k; a NaN never wins
                d2 = v
                step = k
        if step < 0:
            continue                            # gap = +inf: never wins the strict `<` below
        root = math.sqrt(d2)
        gap = root - R
        take = gap < best_gap                   # strict, terms ascending: ties keep the smallest term
        if mutant == "late_term":
            take = gap <= best_gap
        if take:
            best_gap = gap
            best_step = step
            best_code = code
    if best_step < 0:
        return INF, -1, -1
    return best_gap, best_step, best_code


def cross_audit_attached(paths_a, n_a, paths_b, n_b, coupling, pop_a, pop_b, obstacles, rad, separation, right_assoc,
                         mutant=None, full=None):
    """paths_a [Na][cap][3] with n_a [Na] points each, paths_b alike. Returns (clearance, step, sphere), nested lists
    [Na][Nb]. full = (n_a, n_b) of the uncut paths: only the mutant that lets the spheres see past the window reads it."""
    terms = terms_of(coupling, pop_a, pop_b, obstacles, rad, separation, mutant)
    shift = 0 if coupling is None else int(coupling.get("shift", 0))
    la, lb = n_a, n_b
    if mutant == "unwindowed" and full is not None:
        la, lb = full
    a = [[paths_a[i][k] for k in range(int(n_a[i]))] for i in range(len(n_a))]
    b = [[paths_b[j][k] for k in range(int(n_b[j]))] for j in range(len(n_b))]
    clearance, step, sphere = [], [], []
    for i, pa in enumerate(a):
        crow, srow, trow = [], [], []
        for j, pb in enumerate(b):
            if mutant == "unwindowed" and full is not None and len(pa) > 0 and len(pb) > 0:
                # term 0 on the windows, the spheres on the whole paths
                fa = [paths_a[i][k] for k in range(int(la[i]))]
                fb = [paths_b[j][k] for k in range(int(lb[j]))]
                c, s, t = attached_pair(pa, pb, terms[:1], right_assoc)
                c2, s2, t2 = attached_pair(fa, fb, terms[1:], right_assoc)
                if c2 < c:
                    c, s, t = c2, s2, t2
            else:
                c, s, t = attached_pair(pa, pb, terms, right_assoc, mutant, shift)
            crow.append(c)
            srow.append(s)
            trow.append(t)
        clearance.append(crow)
        step.append(srow)
        sphere.append(trow)
    return clearance, step, sphere


def obstacle_side(paths, n_points, obstacles, tracks, first, coupling, pop_a, pop_b, dt, rad, margin, horizon,
                  skip_trailing, right_assoc, mutant=None):
    """(c, fv, w), each [P][N]: pmaf_select_clear_tracked's window audit, population by population, with the columns of
    S_ab left out of pop_a's list and those of S_ba out of pop_b's. tracks: a list over the populations of [L][M][6] or
    None (what the last launched rollout followed), first [P] or None."""
    w = scr.windows(n_points, horizon)
    c, fv = [], []
    for p in range(len(paths)):
        drop = []
        if mutant not in ("columns_kept", "ignored"):
            if p == pop_a:
                drop = attached_columns(coupling, pop_a, pop_b)
            if p == pop_b:
                drop = attached_columns(coupling, pop_b, pop_a)
        M = len(obstacles[p]) - 1
        keep = [s for s in range(M) if s not in drop]
        if skip_trailing and len(keep) == 0:    # nothing left to audit: c = +inf, every agent clear
            c.append([INF for _ in w[p]])
            fv.append(list(w[p]))
            continue
        # the list without the dropped columns (its last row stays the trailing obstacle: the tracked audit drops it
        # itself when skip_trailing), and the tracks' columns to match
        rows = [list(obstacles[p][s]) for s in keep] + [list(obstacles[p][M])]
        trk = None
        if tracks is not None and tracks[p] is not None and len(tracks[p]) > 0:
            trk = [[tracks[p][i][s] for s in keep] for i in range(len(tracks[p]))]
        f = None if first is None else [first[p]]
        r = tar.audit([paths[p]], [n_points[p]], [rows], [trk], f, dt, rad, margin, right_assoc, [w[p]], skip_trailing)
        c.append(r["clearance"][0])
        fv.append(r["first_violation"][0])
    return c, fv, w


def pair_side(paths_a, n_a, paths_b, n_b, coupling, pop_a, pop_b, obstacles, rad, horizon, separation, right_assoc,
              mutant=None):
    """(clearance, step, step, w_a, w_b): the attached audit on the two path sets cut to w = min(n, horizon) points --
    pair_clear_reference.pair_side's tuple"""
    w_a = scr.windows([n_a], horizon)[0]
    w_b = scr.windows([n_b], horizon)[0]
    clearance, step, _ = cross_audit_attached(paths_a, w_a, paths_b, w_b, coupling, pop_a, pop_b, obstacles, rad,
                                              separation, right_assoc, mutant, (n_a, n_b))
    return clearance, step, step, w_a, w_b


def select_pair_clear_tracked(paths, n_points, obstacles, tracks, first, coupling, costs, dt, rad, pop_a, pop_b,
                              obstacle_margin, horizon, skip_trailing, separation, pair_margin, prev_pair, right_assoc,
                              audited=None, matrix=None, mutant=None):
    """pmaf_select_pair_clear_tracked: pair_clear_reference.select_pair_clear's dict. audited / matrix: what
    obstacle_side / pair_side returned for the same inputs (computed once, shared, never modified)."""
    if audited is None:
        audited = obstacle_side(paths, n_points, obstacles, tracks, first, coupling, pop_a, pop_b, dt, rad,
                                obstacle_margin, horizon, skip_trailing, right_assoc, mutant)
    if matrix is None:
        matrix = pair_side(paths[pop_a], n_points[pop_a], paths[pop_b], n_points[pop_b], coupling, pop_a, pop_b,
                           obstacles, rad, horizon, separation, right_assoc, mutant)
    return pcr.select_pair_clear(paths, n_points, obstacles, costs, dt, rad, pop_a, pop_b, obstacle_margin, horizon,
                                 skip_trailing, separation, pair_margin, None, prev_pair, right_assoc, audited, matrix)
