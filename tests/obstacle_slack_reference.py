"""Reference of the audits against the live list with timing slack (include/pmaf.h: pmaf_evaluate_paths_slack,
pmaf_select_clear_slack), written from their stated contract and nothing else. Plain Python floats, one operation per
line: the pair clearance is path_audit_reference.clearance_pair, the list's chain path_audit_reference.obstacle_track,
the track point tracked_audit_reference.point_index, the rule select_clear_reference.select_clear's. Test
infrastructure: it imports neither the oracle nor the package. Every case is decidable, so callers compare every output
at tolerance 0.

MUTANTS name the ways an implementation can misread the contract; tests/test_obstacle_slack_audit.py shows that each of
them changes an output in every shape group the GPU suite runs."""
import path_audit_reference as par
import select_clear_reference as sel
import tracked_audit_reference as tref

INF = float("inf")
MUTANTS = ("band_swapped",       # late and early exchanged
           "late_narrow",        # the band one too narrow on the late side
           "early_narrow",       # ... on the early side
           "no_slack",           # the slack ignored: l = k
           "hold_first",         # the hold applied before the slack: point min(f + k, L-1) + (l - k)
           "multiplied",         # the list's line multiplied out: o^0 + l * RN(v dt)
           "trailing_at_k",      # the trailing obstacle left at the arm's step k
           "fv_reports_l",       # first_violation reports the obstacles' index
           "ties_lk",            # ties ordered (c, l, k, j)
           "negative_l")         # l < 0 admitted, as point 0
KEYS = ("clearance", "step", "obstacle_step", "obstacle", "first_violation")


def clamp_slack(late, early, cap):
    """the host's clamp: a slack of max_prediction_steps or more is max_prediction_steps"""
    late = int(late)
    early = int(early)
    assert late >= 0 and early >= 0
    if late > cap:
        late = cap
    if early > cap:
        early = cap
    return late, early


def band(late, early, mutant=None):
    if mutant == "band_swapped":
        return early, late
    if mutant == "late_narrow":
        return max(late - 1, 0), early
    if mutant == "early_narrow":
        return late, max(early - 1, 0)
    if mutant == "no_slack":
        return 0, 0
    return late, early


def multiplied_line(obstacles, dt, n_idx):
    """(mutant) o^0 + l * RN(v dt) instead of the chain"""
    dt = float(dt)
    out = []
    for l in range(n_idx):
        row = []
        for o in obstacles:
            sx = float(o[3]) * dt
            sy = float(o[4]) * dt
            sz = float(o[5]) * dt
            row.append((float(o[0]) + l * sx, float(o[1]) + l * sy, float(o[2]) + l * sz))
        out.append(row)
    return out


class Positions:
    """o_j^l of one population: obstacles rows (px py pz vx vy vz r) with the trailing one last, tracks [L][M][6] or None /
    empty, the offset `first`; the chain is walked once for n_idx indices and shared"""

    def __init__(self, obstacles, tracks, first, dt, n_idx, mutant=None):
        self.line = par.obstacle_track(obstacles, dt, n_idx)
        if mutant == "multiplied":
            self.line = multiplied_line(obstacles, dt, n_idx)
        self.tracks = tracks
        self.L = 0 if tracks is None else len(tracks)
        self.first = first
        self.M = len(obstacles) - 1
        self.mutant = mutant

    def at(self, k, l, j):
        """obstacle j at the obstacles' index l >= 0, for the arm's step k (which only mutants read)"""
        if self.L > 0 and j < self.M:
            i = tref.point_index(self.first, l, self.L)
            if self.mutant == "hold_first":
                i = tref.point_index(self.first, k, self.L) + (l - k)
                if i > self.L - 1:
                    i = self.L - 1
                if i < 0:
                    i = 0
            pt = self.tracks[i][j]
            return (float(pt[0]), float(pt[1]), float(pt[2]))
        if self.mutant == "trailing_at_k" and j == self.M:
            return self.line[k][j]
        return self.line[l][j]


def audit_path(path, obstacles, pos, rad, margin, late, early, right_assoc, n_audit, mutant=None):
    """path: the w points of ONE agent's window. Returns (clearance, step, obstacle_step, obstacle, first_violation)."""
    w = len(path)
    late, early = band(late, early, mutant)
    rr = []
    for o in obstacles:
        rr.append(float(rad) + float(o[6]))
    margin = float(margin)
    best = INF
    key = None
    won = (-1, -1, -1)
    fv = w
    fv_l = None
    for k in range(w):
        x = (float(path[k][0]), float(path[k][1]), float(path[k][2]))
        for l in range(k - early, k + late + 1):
            idx = l
            if l < 0:
                if mutant != "negative_l":
                    continue
                idx = 0
            for j in range(n_audit):
                c = par.clearance_pair(x, pos.at(k, idx, j), rr[j], right_assoc)
                this = (k, l, j)
                if mutant == "ties_lk":
                    this = (l, k, j)
                if c < best or (c == best and c < INF and this < key):   # the total order (c, k, l, j); NaN never wins
                    best = c
                    key = this
                    won = (k, l, j)
                if c < margin:
                    if fv == w:
                        fv = k       # k ascends: the smallest
                    if fv_l is None or l < fv_l:
                        fv_l = l
    if mutant == "fv_reports_l" and fv_l is not None:
        fv = fv_l
    return best, won[0], won[1], won[2], fv


def audit(paths, n_points, obstacles, tracks, first, dt, rad, margin, late, early, right_assoc, windows=None,
          skip_trailing=False, mutant=None):
    """pmaf_evaluate_paths_slack: paths [P][N][cap][3], n_points [P][N], obstacles [P][n_obs][7], tracks a list over the
    populations of [L][M][6] or None, first [P] or None (zeros). Returns a dict of [P][N] lists (KEYS). windows [P][N]: the
    paths are cut to that many points (the selection); skip_trailing: the lists' last obstacle is not audited (the
    selection only)."""
    out = {k: [] for k in KEYS}
    for p in range(len(paths)):
        lens = n_points[p] if windows is None else windows[p]
        cap = len(paths[p][0])
        lt, ea = clamp_slack(late, early, cap)
        longest = max([int(v) for v in lens] + [0])
        obs = [[float(v) for v in o] for o in obstacles[p]]
        f = 0 if first is None else first[p]
        pos = Positions(obs, None if tracks is None else tracks[p], f, dt, longest + max(lt, ea) + 1, mutant)
        n_audit = len(obs) - 1 if skip_trailing else len(obs)
        rows = {k: [] for k in KEYS}
        for a in range(len(paths[p])):
            n = int(lens[a])
            pts = [paths[p][a][k] for k in range(n)]
            r = audit_path(pts, obs, pos, rad, margin, lt, ea, right_assoc, n_audit, mutant)
            for key, v in zip(KEYS, r):
                rows[key].append(v)
        for k in KEYS:
            out[k].append(rows[k])
    return out


def window_audit(paths, n_points, obstacles, tracks, first, dt, rad, margin, horizon, skip_trailing, late, early,
                 right_assoc, mutant=None):
    """(c, fv, w), each [P][N]: the slacked audit's clearance and first_violation on the paths cut to w = min(n, horizon)"""
    w = sel.windows(n_points, horizon)
    r = audit(paths, n_points, obstacles, tracks, first, dt, rad, margin, late, early, right_assoc, w, skip_trailing, mutant)
    return r["clearance"], r["first_violation"], w


def select_clear(paths, n_points, obstacles, tracks, first, costs, dt, rad, margin, horizon, skip_trailing, late, early,
                 right_assoc, prev=None, audited=None, mutant=None):
    """pmaf_select_clear_slack: select_clear_reference.select_clear's dict. audited: the (c, fv, w) window_audit returned
    for the same arguments (computed once, shared, never modified)."""
    if audited is None:
        audited = window_audit(paths, n_points, obstacles, tracks, first, dt, rad, margin, horizon, skip_trailing, late,
                               early, right_assoc, mutant)
    return sel.select_clear(paths, n_points, obstacles, costs, dt, rad, margin, horizon, right_assoc, prev, audited=audited)
