"""Reference of the selection against the live list (include/pmaf.h: pmaf_select_clear), written from its stated
contract and nothing else. Plain Python: the paths are cut to the audit window and handed to
path_audit_reference.audit (the yardstick the contract names), then the rule is applied one comparison per line. Test
infrastructure: it imports neither the oracle nor the package. Every case is decidable, so callers compare every output
at tolerance 0."""
import path_audit_reference as par

INF = float("inf")


def windows(n_points, horizon):
    """w = min(n, horizon) per agent, [P][N]"""
    out = []
    for row in n_points:
        ws = []
        for n in row:
            n = int(n)
            w = n
            if horizon < w:
                w = horizon
            ws.append(w)
        out.append(ws)
    return out


def window_audit(paths, n_points, obstacles, dt, rad, margin, horizon, right_assoc):
    """(c, fv, w), each [P][N]: pmaf_evaluate_paths' clearance and first_violation on the paths cut to w points"""
    w = windows(n_points, horizon)
    r = par.audit(paths, w, obstacles, dt, rad, margin, right_assoc)
    return r["clearance"], r["first_violation"], w


def pick(cost, fv, w, c, prev=None):
    """The rule for ONE population: cost, fv, w, c are lists over the agents; prev = the previous pick, -1 or None.
    Returns (pick, rule, n_clear)."""
    n = len(cost)
    clear = []
    for a in range(n):
        clear.append(fv[a] == w[a])
    n_clear = 0
    for a in range(n):
        if clear[a]:
            n_clear = n_clear + 1
    # the cheapest clear agent: strict `<` from +infinity over ascending index
    m = -1
    best = INF
    for a in range(n):
        if clear[a]:
            if cost[a] < best:
                best = cost[a]
                m = a
    if m >= 0:
        if prev is not None:
            q = int(prev)
            if q >= 0:
                if clear[q]:
                    if cost[m] >= 0.9 * cost[q]:   # false for a NaN cost of q: it is not kept
                        return q, 0, n_clear
        return m, 1, n_clear
    # fallback: the agent that stays clear longest; greatest fv, then greatest c, then smallest index
    p = 0
    for a in range(1, n):
        if fv[a] > fv[p]:
            p = a
        elif fv[a] == fv[p]:
            if c[a] > c[p]:
                p = a
    return p, 2, n_clear


def select_clear(paths, n_points, obstacles, costs, dt, rad, margin, horizon, right_assoc, prev=None, audited=None):
    """paths [P][N][cap][3], n_points [P][N], obstacles [P][n_obs][7], costs [P][N], prev [P] or None. Returns a dict of
    lists over the populations: pick, rule, n_clear, cost, clearance, first_violation. audited: the (c, fv, w) that
    window_audit returned for the same paths, list, margin and horizon (computed once, shared, never modified)."""
    if audited is None:
        audited = window_audit(paths, n_points, obstacles, dt, rad, margin, horizon, right_assoc)
    c, fv, w = audited
    out = {k: [] for k in ("pick", "rule", "n_clear", "cost", "clearance", "first_violation")}
    for p in range(len(paths)):
        cost = [float(v) for v in costs[p]]
        q = None if prev is None else prev[p]
        i, rule, n_clear = pick(cost, fv[p], w[p], c[p], q)
        out["pick"].append(i)
        out["rule"].append(rule)
        out["n_clear"].append(n_clear)
        out["cost"].append(cost[i])
        out["clearance"].append(c[p][i])
        out["first_violation"].append(fv[p][i])
    return out
