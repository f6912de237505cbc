"""The composed CPU model of one handle's lifetime (include/pmaf.h: repulsive track, obstacle tracks, their couplings, the
tracked audits, the clear selections, pmaf_adopt_best): ModelHandle owns one oracle planner per population and the
handle's INPUT state -- uploads, couplings, offsets, what was taken at the capture moment, what the device buffers hold --
and dispatches every call to the per-feature references, which stay the only place where a value is computed:
field_track_reference.compose (a rollout), sentinel_track_reference.coupled_track, field_couple_reference.compose_tracks,
tracked_audit_reference.audit / select_clear, select_clear_reference.select_clear, path_audit_reference.audit,
pair_clear_reference.select_pair_clear, cross_audit_reference.cross_audit. What the model adds is ORDER: which buffer,
length and offset a launch or an audit is handed after a particular sequence of calls.

The input state is kept the way the contract describes the device's: per population the repulsive points the next launch
follows (`rep_dev`), the obstacle tracks and offsets (`ft_dev`, `ft_first`) -- the getters and the tracked audits read
exactly these --, beside the caller's uploads and couplings they are rebuilt from.

Methods carry PmafPlanner's names and arguments and return the same shapes (P >= 2: nothing is squeezed). A call the
contract refuses raises ModelError with the contract's code and leaves the model unchanged. `mutant=` breaks exactly one
rule of order (MUTANTS); tests/test_sequence_model.py shows that the committed sequences tell each from the model.

Test infrastructure: imports neither the package nor the oracle; both are handed in."""
import copy

import numpy as np

import cross_audit_reference as car
import field_couple_reference as cref
import field_track_reference as fref
import pair_clear_reference as pcr
import path_audit_reference as par
import select_clear_reference as scr
import sentinel_track_reference as sref
import tracked_audit_reference as tar

ERR_INVALID, ERR_STATE = -1, -3
MUTANTS = ("detach_keeps_length", "upload_keeps_offset", "upload_wins_over_coupling", "take_at_launch_in_five_call",
           "take_before_adopt", "set_initial_keeps_taken", "getter_reads_attached", "coupled_audit_reads_next",
           "grow_drops_neighbour", "blob_carries_tracks", "audit_moves_offset", "adopt_ignored_by_real_step",
           # the one rule the sequences found broken in the library (tests/test_sentinel_track_gpu.py has the regression case):
           # an upload between pmaf_reset_agents and pmaf_start dropped what the reset had taken for the coupled populations
           "upload_drops_taken")
LAYOUT = (6, 1, 2, 3, 4)     # pmaf_create's default agent types: Had, Goal, Obstacle, GoalObstacle, Vel, then Random (5)


class ModelError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("model status %d: %s" % (code, msg))
        self.code = code


class _Planner:
    """what a checkpoint blob moves: the oracle planners and the flags that decide refusals"""

    def __init__(self, orc, scs):
        self.oras = [orc.OraclePlanner(sc, mgr_init_pos=sc["start"]) for sc in scs]
        self.reached = [np.asarray(o.success()).copy() for o in self.oras]
        self.obs_start = [np.array(sc["obstacles"], dtype=np.float64) for sc in scs]
        self.stepped = False
        self.rollout_pending = True
        self.eval_best = None       # pmaf_evaluate's own selection of the running tick (the mutants' wrong moment)
        self.pre_adopt = None       # per population the best agent an adoption replaced, until the next evaluate


class _Inputs:
    """what belongs to the handle and never travels in a blob"""

    def __init__(self, P, M):
        self.rep_up = [np.zeros((0, 3)) for _ in range(P)]         # the caller's upload, cut to the capacity
        self.rep_src, self.rep_shift = None, 0                     # pmaf_couple_tracks
        self.rep_dev = [np.zeros((0, 3)) for _ in range(P)]        # what the next launch follows / the getter shows
        self.rep_captured = False
        self.ft_len = [0] * P                                      # the host's lengths of the uploads
        self.ft_dev = [np.zeros((0, M, 6)) for _ in range(P)]
        self.ft_first = [0] * P
        self.ft_stride = 0
        self.fc = None                                             # (src [P][M], scale [P][M], anchor [P][M][3], shift)
        self.fc_pops = [False] * P
        self.f_taken, self.f_captured = None, False

    def rep_uploaded(self):
        return any(len(t) > 0 for t in self.rep_up)

    def rep_on(self):
        return self.rep_uploaded() or self.rep_src is not None

    def ft_attached(self):
        return any(n > 0 for n in self.ft_len)

    def ft_on(self):
        return self.ft_attached() or self.fc is not None


class ModelHandle:
    def __init__(self, orc, scs, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.orc, self.scs, self.mutant = orc, scs, mutant
        self.order = orc.eval_order()
        self.P = len(scs)
        self.N = int(scs[0]["n_agents"])
        self.n_obs = int(scs[0]["obstacles"].shape[0])
        self.M = self.n_obs - 1
        self.cap = int(scs[0]["max_prediction_steps"])
        self.dt = float(scs[0]["dt"])
        self.rad = float(scs[0].get("radius", 0.05))
        self.pl = _Planner(orc, scs)
        self.inp = _Inputs(self.P, self.M)

    def close(self):
        pass

    # ---- plumbing ----------------------------------------------------------------------------------------------------
    def _pos(self, a):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.P, 3)))

    def _obs(self, obstacles):
        return np.asarray(obstacles, dtype=np.float64).reshape(self.P, self.n_obs, 7)

    def _ids(self, a):
        return [int(v) for v in np.broadcast_to(np.asarray(a, dtype=np.int64), (self.P,))]

    def _has_best(self, p):
        return self.pl.oras[p].best_id() > 0

    def _agent_type(self, p, a):
        types = self.scs[p].get("agent_types")
        if types is not None:
            return int(types[a])
        return LAYOUT[a] if a < 5 else 5

    def _tables(self):
        pn = [o.paths() for o in self.pl.oras]
        return ([p.tolist() for p, _ in pn], [n.tolist() for _, n in pn], [o.costs().tolist() for o in self.pl.oras])

    def _snapshot(self):
        """every population's selected path as it lies now: (paths [P], n [P], has_best [P])"""
        sel_p, sel_n, hb = [], [], []
        for p, ora in enumerate(self.pl.oras):
            paths, n = ora.paths()
            has = self._has_best(p)
            b = ora.best_id() - 1 if has else 0
            if self.mutant == "take_before_adopt" and self.pl.eval_best is not None and has:
                b = int(self.pl.eval_best[p])
            sel_p.append(paths[b].copy())
            sel_n.append(int(n[b]))
            hb.append(has)
        return sel_p, sel_n, hb

    # ---- the repulsive track -------------------------------------------------------------------------------------------
    def _rep_coupled(self, p):
        i = self.inp
        if i.rep_src is None or i.rep_src[p] < 0:
            return False
        return not (self.mutant == "upload_wins_over_coupling" and len(i.rep_up[p]) > 0)

    def _rep_rebuild(self):
        """the device buffer from the upload; a coupled population has L = 0 until its track is taken -- unless the
        tracks were taken already (pmaf_reset_agents) and the launch that follows them is still to come"""
        i = self.inp
        for p in range(self.P):
            if self._rep_coupled(p):
                if not i.rep_captured or self.mutant == "upload_drops_taken":
                    i.rep_dev[p] = np.zeros((0, 3))
            else:
                i.rep_dev[p] = i.rep_up[p]

    def _rep_capture(self, snap):
        i = self.inp
        for p in range(self.P):
            if self._rep_coupled(p):
                q = i.rep_src[p]
                i.rep_dev[p] = sref.coupled_track(snap[0][q], snap[1][q], snap[2][q], i.rep_shift)

    def set_repulsive_track(self, tracks, lengths=None):
        assert lengths is None
        i = self.inp
        if tracks is None:
            tracks = [None] * self.P
        assert len(tracks) == self.P
        up = [np.zeros((0, 3)) if t is None else np.array(t, dtype=np.float64).reshape(-1, 3)[:self.cap] for t in tracks]
        i.rep_up = up
        if i.rep_on():
            self._rep_rebuild()
        elif self.mutant != "detach_keeps_length":
            i.rep_dev = [np.zeros((0, 3)) for _ in range(self.P)]

    def couple_tracks(self, src_pop, shift=0):
        i = self.inp
        src = None
        if src_pop is not None:
            if shift < 0:
                raise ModelError(ERR_INVALID, "couple_tracks: shift < 0")
            src = self._ids(src_pop)
            for p, q in enumerate(src):
                if q >= self.P or q == p:
                    raise ModelError(ERR_INVALID, "couple_tracks: src_pop")
            src = [q if q >= 0 else -1 for q in src]
            if all(q < 0 for q in src):
                src = None
        i.rep_src, i.rep_shift = src, (int(shift) if src is not None else 0)
        i.rep_captured = False
        if i.rep_on():
            self._rep_rebuild()
        elif self.mutant != "detach_keeps_length":
            i.rep_dev = [np.zeros((0, 3)) for _ in range(self.P)]

    def get_repulsive_track(self):
        i = self.inp
        if not i.rep_on():
            return [np.zeros((0, 3)) for _ in range(self.P)]
        out = [t.copy() for t in i.rep_dev]
        if self.mutant == "getter_reads_attached":
            snap = self._snapshot()
            for p in range(self.P):
                if self._rep_coupled(p):
                    q = i.rep_src[p]
                    out[p] = sref.coupled_track(snap[0][q], snap[1][q], snap[2][q], i.rep_shift)
        return out

    # ---- the obstacle tracks -------------------------------------------------------------------------------------------
    def _coupled(self, p):
        return self.inp.fc is not None and self.inp.fc_pops[p]

    def _compose_for(self, p, taken):
        src, scale, anchor, shift = self.inp.fc
        return cref.compose_tracks(taken[0], taken[1], taken[2], src[p], scale[p], anchor[p], shift, self.pl.obs_start[p],
                                   self.dt, self.cap)

    def _drop(self, pops):
        """the mutant's grow: what the buffer held for these populations is gone (their lengths stay)"""
        for p in pops:
            self.inp.ft_dev[p] = np.zeros_like(self.inp.ft_dev[p])

    def set_obstacle_tracks(self, tracks, lengths=None):
        assert lengths is None
        i, M = self.inp, self.M
        if tracks is None:
            tracks = [None] * self.P
        assert len(tracks) == self.P
        up = [np.zeros((0, M, 6)) if t is None else np.array(t, dtype=np.float64).reshape(-1, M, 6) for t in tracks]
        for p in range(self.P):
            if len(up[p]) > 0 and self._coupled(p):
                raise ModelError(ERR_INVALID, "set_obstacle_tracks: population %d is coupled" % p)
        any_ = any(len(t) > 0 for t in up)
        max_len = max(1, max(len(t) for t in up))
        keep_first = self.mutant == "upload_keeps_offset"
        i.ft_len = [len(t) for t in up]
        if i.fc is not None:
            if any_ and max_len > i.ft_stride:
                if self.mutant == "grow_drops_neighbour" and i.ft_stride > 0:
                    self._drop([p for p in range(self.P) if self._coupled(p)])
                i.ft_stride = max_len
            for p in range(self.P):
                if not self._coupled(p):
                    i.ft_dev[p] = up[p]
                    if not keep_first:
                        i.ft_first[p] = 0
            return
        i.ft_dev = up
        if not keep_first:
            i.ft_first = [0] * self.P
        if any_:
            i.ft_stride = max(i.ft_stride, max_len)

    def set_obstacle_track_offset(self, first):
        i = self.inp
        f = self._ids(first)
        if any(v < 0 for v in f):
            raise ModelError(ERR_INVALID, "set_obstacle_track_offset: first < 0")
        if not i.ft_on():
            raise ModelError(ERR_STATE, "set_obstacle_track_offset: no obstacle tracks are attached")
        for p in range(self.P):
            if f[p] != 0 and self._coupled(p):
                raise ModelError(ERR_INVALID, "set_obstacle_track_offset: population %d is coupled" % p)
        i.ft_first = f

    def couple_obstacle_tracks(self, src_pop, scale=None, anchor=None, shift=0):
        i, P, M = self.inp, self.P, self.M
        pc = [False] * P
        if src_pop is not None:
            if shift < 0:
                raise ModelError(ERR_INVALID, "couple_obstacle_tracks: shift < 0")
            src = np.ascontiguousarray(np.broadcast_to(np.asarray(src_pop, dtype=np.int64), (P, M)))
            sc = np.ascontiguousarray(np.broadcast_to(np.asarray(1.0 if scale is None else scale, dtype=np.float64), (P, M)))
            an = np.ascontiguousarray(np.broadcast_to(np.asarray(np.zeros(3) if anchor is None else anchor, dtype=np.float64), (P, M, 3)))
            for p in range(P):
                for c in range(M):
                    q = int(src[p, c])
                    if q < -1 or q >= P or q == p:
                        raise ModelError(ERR_INVALID, "couple_obstacle_tracks: src_pop")
                    if q >= 0:
                        pc[p] = True
            for p in range(P):
                if pc[p] and i.ft_len[p] > 0:
                    raise ModelError(ERR_STATE, "couple_obstacle_tracks: population %d has uploaded tracks" % p)
        was = list(i.fc_pops) if i.fc is not None else [False] * P
        i.f_captured = False
        if not any(pc):
            i.fc, i.fc_pops, i.f_taken = None, [False] * P, None
            for p in range(P):
                if was[p]:
                    i.ft_dev[p], i.ft_first[p] = np.zeros((0, M, 6)), 0
            return
        if self.cap > i.ft_stride:
            if self.mutant == "grow_drops_neighbour" and i.ft_stride > 0:
                self._drop([p for p in range(P) if not pc[p]])
            i.ft_stride = self.cap
        i.fc, i.fc_pops, i.f_taken = (src, sc, an, int(shift)), pc, None
        for p in range(P):
            if pc[p] or was[p]:
                i.ft_dev[p], i.ft_first[p] = np.zeros((0, M, 6)), 0

    def _visible_ftracks(self, next_for_coupled=False):
        """(tracks [P], first [P]) as the getter and the tracked audits read them"""
        i = self.inp
        if not i.ft_on():
            return [np.zeros((0, self.M, 6)) for _ in range(self.P)], [0] * self.P
        tr, first = [t.copy() for t in i.ft_dev], list(i.ft_first)
        if next_for_coupled and i.fc is not None:
            snap = self._snapshot()
            for p in range(self.P):
                if self._coupled(p):
                    tr[p] = self._compose_for(p, snap)
        return tr, first

    def get_obstacle_tracks(self):
        tr, first = self._visible_ftracks(self.mutant == "getter_reads_attached")
        return tr, np.asarray(first, dtype=np.int32)

    # ---- the planner's calls -------------------------------------------------------------------------------------------
    def set_initial_position(self, pos):
        pos = self._pos(pos)
        for p, ora in enumerate(self.pl.oras):
            ora.set_initial_position(pos[p])
        if self.mutant != "set_initial_keeps_taken":
            self.inp.rep_captured = False
            self.inp.f_captured = False
        self.pl.rollout_pending = True
        self.pl.stepped = False

    def set_real_position(self, pos):
        pos = self._pos(pos)
        for p, ora in enumerate(self.pl.oras):
            ora.set_real_position(pos[p])

    def set_agent_positions(self, pos):
        pos = self._pos(pos)
        for p, ora in enumerate(self.pl.oras):
            ora.set_agent_positions(pos[p])
        self.pl.rollout_pending = False
        self.pl.stepped = True

    def stop(self):
        pass

    def start(self):
        if self.pl.stepped:
            raise ModelError(ERR_STATE, "start: the agents were set by the stepping API")
        if not self.pl.rollout_pending:
            return
        self._launch(None)

    def _launch(self, pre_snap):
        i, pl = self.inp, self.pl
        snap = [pre_snap]

        def taken_now():
            if snap[0] is None:
                snap[0] = self._snapshot()
            return snap[0]

        if i.fc is not None:
            if not i.f_captured:
                i.f_taken = taken_now()
            i.f_captured = False
            for p in range(self.P):
                if self._coupled(p):
                    i.ft_dev[p], i.ft_first[p] = self._compose_for(p, i.f_taken), 0
        if i.rep_on():
            if i.rep_src is not None and not i.rep_captured:
                self._rep_capture(taken_now())
            i.rep_captured = False
        follow_rep = i.rep_on() or self.mutant == "detach_keeps_length"
        for p, (ora, sc) in enumerate(zip(pl.oras, self.scs)):
            ft = i.ft_dev[p] if i.ft_on() else None
            tr = i.rep_dev[p] if follow_rep else None
            n0 = np.asarray(ora.paths()[1]).copy()
            res = fref.compose(ora, self.order, sc, pl.obs_start[p], ft, i.ft_first[p], tr)
            # (the flag of an agent that took no step is the last rollout's that did: nothing clears it in between)
            ran = np.asarray(res["n_points"]) > n0
            pl.reached[p][ran] = np.asarray(res["reached"])[ran]
        pl.rollout_pending = False

    def evaluate(self, cost_gains, ws):
        best = [ora.evaluate(cost_gains, ws) for ora in self.pl.oras]
        self.pl.eval_best = list(best)
        self.pl.pre_adopt = [None] * self.P
        return np.asarray(best, dtype=np.int32)

    def adopt_best(self, idx):
        ids = self._ids(idx)
        for a in ids:
            if a < -1 or a >= self.N:
                raise ModelError(ERR_INVALID, "adopt_best: index")
        for p, a in enumerate(ids):
            if a < 0:
                continue
            ora = self.pl.oras[p]
            if self.pl.pre_adopt is not None and self.pl.pre_adopt[p] is None and self._has_best(p):
                self.pl.pre_adopt[p] = (ora.best_id(), ora.best_type())
            ora.set_best(a + 1, self._agent_type(p, a), np.asarray(self.scs[p]["random_vecs"])[a])

    def move_real(self, obstacles, dt, steps, agent_id):
        if not all(self._has_best(p) for p in range(self.P)):
            raise ModelError(ERR_STATE, "move_real: no best agent yet")
        obs, ids = self._obs(obstacles), self._ids(agent_id)
        for p, ora in enumerate(self.pl.oras):
            pre = self.pl.pre_adopt[p] if self.pl.pre_adopt is not None else None
            if self.mutant == "adopt_ignored_by_real_step" and pre is not None:
                now = (ora.best_id(), ora.best_type())
                rv = np.asarray(self.scs[p]["random_vecs"])
                ora.set_best(pre[0], pre[1], rv[pre[0] - 1])
                ora.move_real(obs[p], dt, steps, ids[p])
                ora.set_best(now[0], now[1], rv[now[0] - 1])
            else:
                ora.move_real(obs[p], dt, steps, ids[p])

    def reset_agents(self, pos, vel, obstacles):
        pos, vel, obs = self._pos(pos), self._pos(vel), self._obs(obstacles)
        i = self.inp
        if self.mutant != "take_at_launch_in_five_call":
            if i.rep_src is not None or i.fc is not None:
                snap = self._snapshot()
                if i.rep_src is not None:
                    self._rep_capture(snap)
                    i.rep_captured = True
                if i.fc is not None:
                    i.f_taken, i.f_captured = snap, True
        for p, ora in enumerate(self.pl.oras):
            ora.reset_agents(pos[p], vel[p], obs[p])
            self.pl.obs_start[p] = obs[p].copy()
        self.pl.rollout_pending = True
        self.pl.stepped = False

    def tick(self, obstacles, dt, cost_gains, ws, want_outputs=True):
        obs = self._obs(obstacles)
        best = self.evaluate(cost_gains, ws)
        snap = self._snapshot()      # after the selection, before the reset cuts the paths
        for p, ora in enumerate(self.pl.oras):
            ora.move_real(obs[p], dt, 1, int(best[p]))
            pos, vel, _ = ora.real_state()
            ora.reset_agents(pos, vel, obs[p])
            self.pl.obs_start[p] = obs[p].copy()
        self.pl.stepped = False
        self.pl.rollout_pending = True
        self._launch(snap)
        return best

    def audited_tick(self, obstacles, dt, cost_gains, ws, margin, horizon, prev=None, tracked=False):
        self.stop()
        best = self.evaluate(cost_gains, ws)
        if tracked:
            sel = self.select_clear_tracked(obstacles, margin, horizon, prev=prev, adopt=True)
        else:
            sel = self.select_clear(obstacles, margin, horizon, prev=prev, adopt=True)
        self.move_real(obstacles, dt, 1, sel["pick"])
        pos, vel, _ = self.real_state()
        self.reset_agents(pos, vel, obstacles)
        self.start()
        return dict(sel, best=best)

    # ---- audits and selections ---------------------------------------------------------------------------------------------
    def _prev(self, prev):
        if prev is None:
            return None
        pv = self._ids(prev)
        for q in pv:
            if q < -1 or q >= self.N:
                raise ModelError(ERR_INVALID, "prev_idx")
        return pv

    def _horizon(self, horizon):
        if horizon < 1:
            raise ModelError(ERR_INVALID, "horizon < 1")
        return min(int(horizon), self.cap)

    def evaluate_paths(self, obstacles, margin=0.0, per_obstacle=False):
        paths, n, _ = self._tables()
        r = par.audit(paths, n, self._obs(obstacles).tolist(), self.dt, self.rad, margin, self.order)
        return self._audit_dict(r, per_obstacle)

    @staticmethod
    def _audit_dict(r, per_obstacle):
        out = {"clearance": np.asarray(r["clearance"], dtype=np.float64)}
        for k in ("step", "obstacle", "first_violation"):
            out[k] = np.asarray(r[k], dtype=np.int32)
        if per_obstacle:
            out["per_obstacle"] = np.asarray(r["per_obstacle"], dtype=np.float64)
        return out

    def _tracked_inputs(self, first):
        f = None
        if first is not None:
            f = self._ids(first)
            if any(v < 0 for v in f):
                raise ModelError(ERR_INVALID, "first < 0")
            if not self.inp.ft_on():
                raise ModelError(ERR_STATE, "first given with no obstacle tracks attached")
        tr, own = self._visible_ftracks(self.mutant == "coupled_audit_reads_next")
        return [t.tolist() if len(t) else None for t in tr], (own if f is None else f)

    def _offset_moved_by_audit(self, first):
        if self.mutant == "audit_moves_offset" and first is not None:
            f = self._ids(first)
            for p in range(self.P):
                if not self._coupled(p):
                    self.inp.ft_first[p] = f[p]

    def evaluate_paths_tracked(self, obstacles, margin=0.0, per_obstacle=False, first=None):
        tracks, f = self._tracked_inputs(first)
        paths, n, _ = self._tables()
        r = tar.audit(paths, n, self._obs(obstacles).tolist(), tracks, f, self.dt, self.rad, margin, self.order)
        self._offset_moved_by_audit(first)
        return self._audit_dict(r, per_obstacle)

    @staticmethod
    def _select_dict(r):
        out = {k: np.asarray(r[k], dtype=np.int32) for k in ("pick", "rule", "n_clear", "first_violation")}
        out["cost"], out["clearance"] = np.asarray(r["cost"], dtype=np.float64), np.asarray(r["clearance"], dtype=np.float64)
        return out

    def select_clear(self, obstacles, margin, horizon, prev=None, adopt=False):
        horizon, pv = self._horizon(horizon), self._prev(prev)
        paths, n, costs = self._tables()
        r = scr.select_clear(paths, n, self._obs(obstacles).tolist(), costs, self.dt, self.rad, margin, horizon, self.order, pv)
        if adopt:
            self.adopt_best(r["pick"])
        return self._select_dict(r)

    def select_clear_tracked(self, obstacles, margin, horizon, prev=None, adopt=False, first=None, skip_trailing=False):
        horizon, pv = self._horizon(horizon), self._prev(prev)
        tracks, f = self._tracked_inputs(first)
        paths, n, costs = self._tables()
        r = tar.select_clear(paths, n, self._obs(obstacles).tolist(), tracks, f, costs, self.dt, self.rad, margin, horizon,
                             bool(skip_trailing), self.order, pv)
        if adopt:
            self.adopt_best(r["pick"])
        else:
            self._offset_moved_by_audit(first)
        return self._select_dict(r)

    def select_pair_clear(self, pop_a, pop_b, obstacles, obstacle_margin, horizon, separation, pair_margin,
                          skip_trailing=False, late=None, prev_pair=None, adopt=False):
        if pop_a == pop_b or not (0 <= pop_a < self.P and 0 <= pop_b < self.P):
            raise ModelError(ERR_INVALID, "select_pair_clear: populations")
        horizon = self._horizon(horizon)
        if late is not None and (late[0] < 0 or late[1] < 0):
            raise ModelError(ERR_INVALID, "select_pair_clear: late")
        paths, n, costs = self._tables()
        r = pcr.select_pair_clear(paths, n, self._obs(obstacles).tolist(), costs, self.dt, self.rad, pop_a, pop_b,
                                  obstacle_margin, horizon, bool(skip_trailing), separation, pair_margin,
                                  None if late is None else (int(late[0]), int(late[1])), prev_pair, self.order)
        if adopt and r["pair"][0] >= 0:
            ids = [-1] * self.P
            ids[pop_a], ids[pop_b] = r["pair"]
            self.adopt_best(ids)
        return r

    def cross_audit(self, pop_a, pop_b, separation, step=False):
        if pop_a == pop_b or not (0 <= pop_a < self.P and 0 <= pop_b < self.P):
            raise ModelError(ERR_INVALID, "cross_audit: populations")
        paths, n, _ = self._tables()
        clr, st = car.cross_audit(paths[pop_a], n[pop_a], paths[pop_b], n[pop_b], separation, self.order)
        clr, st = np.asarray(clr, dtype=np.float64), np.asarray(st, dtype=np.int32)
        return (clr, st) if step else clr

    # ---- the checkpoint ----------------------------------------------------------------------------------------------------
    def save_state(self):
        """the blob: the planner state (handed on, not copied: the saving handle is closed afterwards)"""
        return {"planner": self.pl, "inputs": copy.deepcopy(self.inp)}

    def load_state(self, blob):
        self.pl = blob["planner"]
        if self.mutant == "blob_carries_tracks":
            self.inp = blob["inputs"]

    # ---- getters -----------------------------------------------------------------------------------------------------------
    def paths(self):
        pn = [o.paths() for o in self.pl.oras]
        return np.stack([p for p, _ in pn]), np.stack([n for _, n in pn]).astype(np.int32)

    def n_points(self):
        return self.paths()[1]

    def costs(self):
        return np.stack([o.costs() for o in self.pl.oras])

    def rot_vecs(self):
        return np.stack([o.rot_vecs() for o in self.pl.oras])

    def known(self):
        return np.stack([o.known() for o in self.pl.oras]).astype(np.int32)

    def min_obs_dist(self):
        return np.stack([o.min_obs_dist() for o in self.pl.oras])

    def success(self):
        return np.stack(self.pl.reached).astype(np.int32)

    def agent_vel(self):
        return np.stack([o.agent_vel() for o in self.pl.oras])

    def real_state(self):
        st = [o.real_state() for o in self.pl.oras]
        return tuple(np.stack([s[k] for s in st]) for k in range(3))

    def best(self):
        return (np.asarray([o.best_type() for o in self.pl.oras], dtype=np.int32),
                np.asarray([o.best_id() for o in self.pl.oras], dtype=np.int32))
