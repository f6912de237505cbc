"""Reference of the joint selection (include/pmaf.h: pmaf_select_pair_clear, pmaf_select_clear_tracks), written from
its stated contract by composing three existing references and nothing else: select_clear_reference.window_audit on the
lists (the last row dropped when skip_trailing), cross_audit_reference.cross_audit or
slack_audit_reference.cross_audit_slack on the paths cut to their windows, and the rule as nested row-major scans, one
comparison per line. Plain Python floats. Test infrastructure: it imports neither the oracle nor the package. Every case
is decidable, so callers compare every output at tolerance 0."""
import cross_audit_reference as car
import select_clear_reference as scr
import slack_audit_reference as sar

INF = float("inf")
NAN = float("nan")


def obstacle_side(paths, n_points, obstacles, dt, rad, margin, horizon, skip_trailing, right_assoc):
    """(c, fv, w), each [P][N]: pmaf_select_clear's window audit; with skip_trailing the last obstacle of every list is
    left out, and a list of one obstacle then leaves nothing to audit: c = +inf, every agent clear"""
    lists = [[list(row) for row in pop] for pop in obstacles]
    if skip_trailing:
        lists = [pop[:-1] for pop in lists]
    if len(lists[0]) == 0:
        w = scr.windows(n_points, horizon)
        return [[INF for _ in row] for row in w], [list(row) for row in w], w
    return scr.window_audit(paths, n_points, lists, dt, rad, margin, horizon, right_assoc)


def pair_side(paths_a, n_a, paths_b, n_b, horizon, separation, late, right_assoc):
    """(clearance, step_a, step_b), each [Na][Nb], and the windows (w_a, w_b): the cross audit on the two path sets cut
    to w = min(n, horizon) points; late = None (step against step: step_b = step_a) or (late_a, late_b)"""
    w_a = scr.windows([n_a], horizon)[0]
    w_b = scr.windows([n_b], horizon)[0]
    if late is None:
        clearance, step = car.cross_audit(paths_a, w_a, paths_b, w_b, separation, right_assoc)
        return clearance, step, step, w_a, w_b
    clearance, step_a, step_b = sar.cross_audit_slack(paths_a, w_a, paths_b, w_b, separation, late[0], late[1], right_assoc)
    return clearance, step_a, step_b, w_a, w_b


def excess(ca, cb, clearance, obstacle_margin, pair_margin):
    """g of one pair and whether the pair takes part in rule 2; cb = None: the tracks variant, no gb"""
    ga = ca - obstacle_margin
    g = ga
    if cb is not None:
        gb = cb - obstacle_margin
        if gb < g:
            g = gb
    gp = clearance - pair_margin
    if gp < g:
        g = gp
    return g, not (gp != gp)


def joint_rule(cost_a, cost_b, clear_a, clear_b, c_a, c_b, clearance, obstacle_margin, pair_margin, prev_pair=None):
    """The rule. cost_a [Na], cost_b [Nb]; clear_a [Na], clear_b [Nb] booleans; c_a [Na], c_b [Nb] or None (tracks);
    clearance [Na][Nb]. Returns (pair, rule, n_feasible)."""
    na = len(cost_a)
    nb = len(cost_b)
    obstacle_margin = float(obstacle_margin)
    pair_margin = float(pair_margin)

    def feasible(i, j):
        if not clear_a[i]:
            return False
        if not clear_b[j]:
            return False
        return float(clearance[i][j]) >= pair_margin      # false for a NaN clearance

    def total(i, j):
        return float(cost_a[i]) + float(cost_b[j])

    n_feasible = 0
    m = (-1, -1)
    best = INF
    for i in range(na):
        for j in range(nb):
            if feasible(i, j):
                n_feasible = n_feasible + 1
                s = total(i, j)
                if s < best:                               # strict, row-major; a NaN or +inf sum never wins
                    best = s
                    m = (i, j)
    if m != (-1, -1):
        if prev_pair is not None:
            qi = int(prev_pair[0])
            qj = int(prev_pair[1])
            if qi >= 0 and qj >= 0:
                if feasible(qi, qj):
                    if best >= 0.9 * total(qi, qj):        # false for a NaN sum of the previous pair: it is not kept
                        return (qi, qj), 0, n_feasible
        return m, 1, n_feasible
    pick = (-1, -1)
    best_g = -INF
    for i in range(na):
        for j in range(nb):
            g, takes_part = excess(float(c_a[i]), None if c_b is None else float(c_b[j]), float(clearance[i][j]),
                                   obstacle_margin, pair_margin)
            if not takes_part:
                continue
            if g > best_g:                                 # strict, row-major
                best_g = g
                pick = (i, j)
    if pick != (-1, -1):
        return pick, 2, n_feasible
    return pick, -1, n_feasible


def _result(pair, rule, n_feasible, cost_a, cost_b, clear_a, clear_b, c_a, c_b, fv_a, fv_b, clearance, step_a, step_b,
            obstacle_margin, pair_margin):
    out = {"pair": pair, "rule": rule, "n_feasible": n_feasible,
           "n_clear": (sum(1 for v in clear_a if v), sum(1 for v in clear_b if v))}
    i, j = pair
    if i < 0:
        out.update(cost=NAN, clearance=NAN, obstacle_clearance=(NAN, NAN), first_violation=(-1, -1), worst_excess=NAN,
                   steps=(-1, -1))
        return out
    g, _ = excess(float(c_a[i]), None if c_b is None else float(c_b[j]), float(clearance[i][j]), float(obstacle_margin),
                  float(pair_margin))
    out.update(cost=float(cost_a[i]) + float(cost_b[j]), clearance=float(clearance[i][j]),
               obstacle_clearance=(float(c_a[i]), INF if c_b is None else float(c_b[j])),
               first_violation=(int(fv_a[i]), int(fv_b[j])), worst_excess=g, steps=(int(step_a[i][j]), int(step_b[i][j])))
    return out


def select_pair_clear(paths, n_points, obstacles, costs, dt, rad, pop_a, pop_b, obstacle_margin, horizon, skip_trailing,
                      separation, pair_margin, late, prev_pair, right_assoc, audited=None, matrix=None):
    """paths [P][N][cap][3], n_points [P][N], obstacles [P][n_obs][7], costs [P][N]. audited / matrix: what
    obstacle_side / pair_side returned for the same inputs (computed once, shared, never modified). Returns a dict:
    pair, rule, n_feasible, n_clear (2), cost, clearance, obstacle_clearance (2), first_violation (2), worst_excess,
    steps (2)."""
    if audited is None:
        audited = obstacle_side(paths, n_points, obstacles, dt, rad, obstacle_margin, horizon, skip_trailing, right_assoc)
    if matrix is None:
        matrix = pair_side(paths[pop_a], n_points[pop_a], paths[pop_b], n_points[pop_b], horizon, separation, late, right_assoc)
    c, fv, w = audited
    clearance, step_a, step_b, _, _ = matrix
    clear_a = [fv[pop_a][i] == w[pop_a][i] for i in range(len(w[pop_a]))]
    clear_b = [fv[pop_b][j] == w[pop_b][j] for j in range(len(w[pop_b]))]
    pair, rule, n_feasible = joint_rule(costs[pop_a], costs[pop_b], clear_a, clear_b, c[pop_a], c[pop_b], clearance,
                                        obstacle_margin, pair_margin, prev_pair)
    return _result(pair, rule, n_feasible, costs[pop_a], costs[pop_b], clear_a, clear_b, c[pop_a], c[pop_b], fv[pop_a],
                   fv[pop_b], clearance, step_a, step_b, obstacle_margin, pair_margin)


def select_clear_tracks(paths, n_points, obstacles, costs, dt, rad, pop, obstacle_margin, horizon, skip_trailing, tracks,
                        n_track_points, track_cost, separation, pair_margin, late, prev_pair, right_assoc):
    """the same against the caller's tracks [n_tracks][cap][3]: every track is clear, its first violation is reported as
    its window, its obstacle clearance as +inf, its cost is track_cost[j] or +0.0, and g has no term for it"""
    c, fv, w = obstacle_side(paths, n_points, obstacles, dt, rad, obstacle_margin, horizon, skip_trailing, right_assoc)
    clearance, step_a, step_b, _, w_b = pair_side(paths[pop], n_points[pop], tracks, n_track_points, horizon, separation,
                                                  late, right_assoc)
    nt = len(n_track_points)
    cost_b = [0.0] * nt if track_cost is None else [float(v) for v in track_cost]
    clear_a = [fv[pop][i] == w[pop][i] for i in range(len(w[pop]))]
    clear_b = [True] * nt
    pair, rule, n_feasible = joint_rule(costs[pop], cost_b, clear_a, clear_b, c[pop], None, clearance, obstacle_margin,
                                        pair_margin, prev_pair)
    return _result(pair, rule, n_feasible, costs[pop], cost_b, clear_a, clear_b, c[pop], None, fv[pop], w_b, clearance,
                   step_a, step_b, obstacle_margin, pair_margin)
