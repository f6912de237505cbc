"""Reference of the audits against the obstacle tracks (include/pmaf.h: pmaf_evaluate_paths_tracked,
pmaf_select_clear_tracked), written from their stated contract and nothing else. Plain Python: a composer builds the
obstacle positions track[k][j] -- from the caller's tracks for a tracked field obstacle, from
path_audit_reference.obstacle_track (the list's iterated line) for the trailing obstacle and for a population without
tracks -- and hands them to path_audit_reference.audit_path, with the path cut to the window for the selection; the rule is
select_clear_reference.select_clear's. Test infrastructure: it imports neither the oracle nor the package. Every case is
decidable, so callers compare every output at tolerance 0.

MUTANTS name the ways an implementation can misread the contract; tests/test_tracked_audit.py shows that each of them
changes an output in every shape group the GPU suite runs."""
import path_audit_reference as par
import select_clear_reference as sel

MUTANTS = ("ignore", "kplus", "kminus", "nohold", "first_ignored", "trailing_tracked", "trailing_dropped", "velocity",
           "radius")
KEYS = ("clearance", "step", "obstacle", "first_violation", "per_obstacle")


def point_index(first, k, L, mutant=None):
    """min(first + k, L-1), with first clamped to L-1 before k is added (the same function); None where the (mutant)
    rule leaves the track for the list's line"""
    f = int(first)
    if mutant == "first_ignored":
        f = 0
    last = L - 1
    if f > last:
        f = last
    i = f + k
    if mutant == "kplus":
        i = i + 1
    if mutant == "kminus":
        i = i - 1
        if i < 0:
            i = 0
    if i > last:
        if mutant == "nohold":
            return None
        i = last
    return i


def compose_track(obstacles, tracks, first, dt, n_steps, mutant=None):
    """track[k][j] = (x, y, z) for k < n_steps and every obstacle j of `obstacles` (rows px py pz vx vy vz r).
    tracks: [L][M][6] of the M = len(obstacles) - 1 field obstacles, or None / empty (L == 0)."""
    line = par.obstacle_track(obstacles, dt, n_steps)
    L = 0
    if tracks is not None:
        L = len(tracks)
    if L == 0:
        return line
    if mutant == "ignore":
        return line
    M = len(obstacles) - 1
    dt = float(dt)
    out = []
    for k in range(n_steps):
        row = list(line[k])
        i = point_index(first, k, L, mutant)
        if i is not None:
            for j in range(M):
                pt = tracks[i][j]
                x = float(pt[0])
                y = float(pt[1])
                z = float(pt[2])
                if mutant == "velocity":
                    sx = float(pt[3]) * dt
                    sy = float(pt[4]) * dt
                    sz = float(pt[5]) * dt
                    x = x + sx
                    y = y + sy
                    z = z + sz
                row[j] = (x, y, z)
            if mutant == "trailing_tracked":
                if M > 0:
                    pt = tracks[i][M - 1]
                    row[M] = (float(pt[0]), float(pt[1]), float(pt[2]))
        out.append(row)
    return out


def _rows(obstacles, mutant):
    rows = [[float(v) for v in o] for o in obstacles]
    if mutant == "radius":
        for o in rows[:-1]:
            o[6] = o[6] + 0.03
    return rows


def _tracks_of(tracks, p):
    if tracks is None:
        return None
    return tracks[p]


def _first_of(first, p):
    if first is None:
        return 0
    return first[p]


def audit(paths, n_points, obstacles, tracks, first, dt, rad, margin, right_assoc, windows=None, skip_trailing=False,
          mutant=None):
    """pmaf_evaluate_paths_tracked: paths [P][N][cap][3], n_points [P][N], obstacles [P][n_obs][7], tracks a list over the
    populations of [L][M][6] or None, first [P] or None (zeros). Returns path_audit_reference.audit's dict. windows
    [P][N]: the paths are cut to that many points (the selection); skip_trailing: the lists' last row is dropped before
    the audit (the selection only)."""
    out = {k: [] for k in KEYS}
    if mutant == "trailing_dropped":
        skip_trailing = True
    for p in range(len(paths)):
        lens = n_points[p]
        if windows is not None:
            lens = windows[p]
        longest = max([int(v) for v in lens] + [0])
        obs = _rows(obstacles[p], mutant)
        track = compose_track(obs, _tracks_of(tracks, p), _first_of(first, p), dt, longest, mutant)
        if skip_trailing:
            obs = obs[:-1]
            track = [row[:-1] for row in track]
        rows = {k: [] for k in KEYS}
        for a in range(len(paths[p])):
            n = int(lens[a])
            pts = [paths[p][a][k] for k in range(n)]
            r = par.audit_path(pts, obs, dt, rad, margin, right_assoc, track)
            for key, v in zip(KEYS, r):
                rows[key].append(v)
        for k in KEYS:
            out[k].append(rows[k])
    return out


def window_audit(paths, n_points, obstacles, tracks, first, dt, rad, margin, horizon, skip_trailing, right_assoc,
                 mutant=None):
    """(c, fv, w), each [P][N]: the tracked audit's clearance and first_violation on the paths cut to w = min(n, horizon)"""
    w = sel.windows(n_points, horizon)
    r = audit(paths, n_points, obstacles, tracks, first, dt, rad, margin, right_assoc, w, skip_trailing, mutant)
    return r["clearance"], r["first_violation"], w


def select_clear(paths, n_points, obstacles, tracks, first, costs, dt, rad, margin, horizon, skip_trailing, right_assoc,
                 prev=None, audited=None, mutant=None):
    """pmaf_select_clear_tracked: select_clear_reference.select_clear's dict. audited: the (c, fv, w) window_audit
    returned for the same arguments (computed once, shared, never modified)."""
    if audited is None:
        audited = window_audit(paths, n_points, obstacles, tracks, first, dt, rad, margin, horizon, skip_trailing,
                               right_assoc, mutant)
    return sel.select_clear(paths, n_points, obstacles, costs, dt, rad, margin, horizon, right_assoc, prev, audited)
