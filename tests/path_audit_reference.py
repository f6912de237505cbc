"""Reference of the path audit (include/pmaf.h: pmaf_evaluate_paths), written from its stated semantics and nothing
else: plain Python floats (IEEE double, round to nearest, no fused operations) and math.sqrt (correctly rounded), one
operation per line, in the order the contract gives. Test infrastructure: it imports neither the oracle nor the
package; the caller passes the library's evaluation order (pmaf_eval_order(): 0 = (a0 b0 + a1 b1) + a2 b2,
1 = a0 b0 + (a1 b1 + a2 b2)). Every case is decidable, so callers compare every output at tolerance 0."""
import math

INF = float("inf")


def obstacle_track(obstacles, dt, n_steps):
    """obstacles: rows of (px, py, pz, vx, vy, vz, r). track[k][j] = (x, y, z) with o^0 the given position and
    o^{k+1} = o^k + v * dt per component: one multiply, then one add, each rounded (iterated, not o^0 + k (v dt))."""
    cur = [(float(o[0]), float(o[1]), float(o[2])) for o in obstacles]
    vel = [(float(o[3]), float(o[4]), float(o[5])) for o in obstacles]
    dt = float(dt)
    track = []
    for _ in range(n_steps):
        track.append(cur)
        nxt = []
        for (x, y, z), (vx, vy, vz) in zip(cur, vel):
            sx = vx * dt
            sy = vy * dt
            sz = vz * dt
            nx = x + sx
            ny = y + sy
            nz = z + sz
            nxt.append((nx, ny, nz))
        cur = nxt
    return track


def clearance_pair(x, o, rr, right_assoc):
    """c = norm(x - o) - rr with norm = sqrt(dot(d, d)) in the given association"""
    dx = x[0] - o[0]
    dy = x[1] - o[1]
    dz = x[2] - o[2]
    xx = dx * dx
    yy = dy * dy
    zz = dz * dz
    if right_assoc:
        t = yy + zz
        s = xx + t
    else:
        t = xx + yy
        s = t + zz
    nrm = math.sqrt(s)   # s is >= 0, +inf or NaN: none of them raises; +inf and NaN propagate
    return nrm - rr


def audit_path(path, obstacles, dt, rad, margin, right_assoc, track=None):
    """path: n points (x, y, z) of ONE agent. Returns (clearance, step, obstacle, first_violation, per_obstacle)."""
    n = len(path)
    n_obs = len(obstacles)
    if track is None:
        track = obstacle_track(obstacles, dt, n)
    rr = []
    for o in obstacles:
        rr.append(float(rad) + float(o[6]))
    best = INF
    step = -1
    obstacle = -1
    first_violation = n
    per_obstacle = [INF] * n_obs
    margin = float(margin)
    for k in range(n):
        x = (float(path[k][0]), float(path[k][1]), float(path[k][2]))
        for j in range(n_obs):
            c = clearance_pair(x, track[k][j], rr[j], right_assoc)
            if c < best:              # strict: ties keep the smallest k, then the smallest j; NaN never wins
                best = c
                step = k
                obstacle = j
            if c < per_obstacle[j]:
                per_obstacle[j] = c
            if c < margin and first_violation == n:
                first_violation = k
    if n == 0:
        first_violation = 0
    return best, step, obstacle, first_violation, per_obstacle


def audit(paths, n_points, obstacles, dt, rad, margin, right_assoc):
    """paths [P][N][cap][3], n_points [P][N], obstacles [P][n_obs][7] (anything indexable). Returns a dict of nested
    lists: clearance, step, obstacle, first_violation [P][N] and per_obstacle [P][N][n_obs]."""
    out = {k: [] for k in ("clearance", "step", "obstacle", "first_violation", "per_obstacle")}
    for p in range(len(paths)):
        rows = {k: [] for k in out}
        longest = max([int(v) for v in n_points[p]] + [0])
        track = obstacle_track(obstacles[p], dt, longest)   # computed once per population, shared, never modified
        for a in range(len(paths[p])):
            n = int(n_points[p][a])
            pts = [paths[p][a][k] for k in range(n)]
            r = audit_path(pts, obstacles[p], dt, rad, margin, right_assoc, track)
            for key, v in zip(("clearance", "step", "obstacle", "first_violation", "per_obstacle"), r):
                rows[key].append(v)
        for k in out:
            out[k].append(rows[k])
    return out
