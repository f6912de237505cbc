"""Seeded call sequences over one handle's lifetime, and the loop that runs one on two handles and compares them after
every call: tests/test_sequence_gpu.py (PmafPlanner against sequence_model.ModelHandle), tests/test_sequence_model.py (the
model against its mutants, through the same comparison) and tools/fuzz_sequences.py (seeds beyond SEEDS) share it.

sequence(seed) draws a shape, the number of populations and a list of (op, args) from numpy.random.default_rng(seed) and
nothing else. The generator keeps a shadow of the handle's input state (what is uploaded, what is coupled, whether a
reset waits for its start) and only draws a call the contract accepts, or -- ops named refuse_* -- one whose refusal code
the contract names. Arguments are names and small integers; Context resolves them to arrays (tracks from
field_track_reference.tracks_for / sentinel_track_reference.tracks_for on field_couple_reference's crossing scenes), and
what depends on the run -- the index an adoption takes, the previous pick -- is derived from the handle's own earlier
results, the same way on both sides.

Test infrastructure: imports neither the package nor the oracle; both are handed in."""
import numpy as np

import field_couple_reference as cref
import field_track_reference as fref
import sentinel_track_reference as sref

ERR_INVALID, ERR_STATE = -1, -3
SHAPES = ("M3-cap9", "M3-cap70", "M59-cap9-general-moving", "M60-cap70-lds-general-moving")
MAX_TICKS = 10

TICK_OPS = ("tick", "tick5", "tick5_adopt_best", "tick5_select_clear", "tick5_select_clear_tracked", "audited_tick",
            "audited_tick_tracked", "reset5", "start")
INPUT_OPS = ("set_repulsive_track", "couple_tracks", "set_obstacle_tracks", "set_obstacle_track_offset",
             "couple_obstacle_tracks", "set_initial_position", "set_real_position", "handover")
READ_OPS = ("get_repulsive_track", "get_obstacle_tracks", "evaluate_paths", "evaluate_paths_tracked", "select_clear",
            "select_clear_tracked", "select_pair_clear", "cross_audit")
REFUSALS = {  # op -> the code include/pmaf.h names
    "refuse_couple_field_on_uploaded": ERR_STATE,
    "refuse_upload_on_coupled": ERR_INVALID,
    "refuse_offset_on_coupled": ERR_INVALID,
    "refuse_offset_without_tracks": ERR_STATE,
    "refuse_couple_self": ERR_INVALID,
    "refuse_couple_range": ERR_INVALID,
    "refuse_negative_shift": ERR_INVALID,
    "refuse_start_after_stepping": ERR_STATE,
}
OTHER_OPS = ("set_agent_positions",)      # the stepping call in front of refuse_start_after_stepping
ALPHABET = TICK_OPS + INPUT_OPS + READ_OPS + tuple(REFUSALS) + OTHER_OPS
# the ticks that launch a rollout (reset5 launches none: its start does)
LAUNCHING = ("tick", "tick5", "tick5_adopt_best", "tick5_select_clear", "tick5_select_clear_tracked", "audited_tick",
             "audited_tick_tracked", "start")

MARGINS = (0.0, 0.02, 0.06)
HORIZONS = (1, 5, 30, 500)
SEPARATIONS = (0.1, 0.2)
LATES = (None, (0, 0), (2, 1))
SCALES = (1.0, 0.8, 0.9)
ANCHORS = ((-0.25, 0.0, 0.0), (0.0, 0.0, 0.0), (-0.03, 0.02, 0.0), (0.0, 0.75, 0.05))
DELTAS = ((0.0, 0.0, 0.0), (0.01, -0.005, 0.0), (-0.004, 0.002, 0.003))
# a measured position 0.22 m ahead of / behind the set-point: more than 0.2 m from the initial position the real agent's
# gate is open, its next step latches the obstacles in its shell with the BEST agent's heuristic -- where an adoption shows
JUMPS = ((0.22, 0.02, 0.0), (-0.22, -0.02, 0.0))
LENGTH_NAMES = ("L1", "L2", "Lcap", "Lcap+5", "short")
STATE_FIELDS = ("paths", "n_points", "costs", "rot_vecs", "known", "min_obs_dist", "success", "agent_vel", "real_state",
                "best", "get_repulsive_track", "get_obstacle_tracks")


# ---- the generator ----------------------------------------------------------------------------------------------------
class _Shadow:
    def __init__(self, P):
        self.P = P
        self.reset()
        self.launched = False        # a rollout has run: there are paths to audit
        self.selected = False        # a selection has been made: there are costs, and move_real is allowed
        self.waiting = False         # reset5 went through, its start has not
        self.restarted = False       # the paths were restarted after a rollout: a tick comes next, not a bare start
        self.jumped = False          # the measured position is one JUMP ahead
        self.ticks = 0
        self.last_long = False       # the last repulsive / obstacle upload was a long one

    def reset(self):
        P = self.P
        self.rep = [None] * P        # names of the uploaded repulsive tracks
        self.rep_src = None
        self.ft = [None] * P         # names of the uploaded obstacle tracks
        self.fc = [False] * P        # populations with a coupled column

    def ft_on(self):
        return any(self.ft) or any(self.fc)


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _names(rng, P, coupled=None, want_long=None):
    """per population a track name or None; never all None, never one for a coupled population"""
    free = [p for p in range(P) if not (coupled and coupled[p])]
    out = [None] * P
    some = [p for p in free if rng.integers(0, 3) > 0] or free[:1]
    for p in some:
        if want_long is None:
            out[p] = _pick(rng, LENGTH_NAMES)
        else:
            out[p] = _pick(rng, ("Lcap", "Lcap+5")) if want_long else _pick(rng, ("L1", "L2", "short"))
    return tuple(out)


def _first_specs(rng, sh, for_audit=False):
    """per population an offset: 0, 1, L - 1 or L + 3 of what it has uploaded; 0 for a coupled one (the audits may pass
    any number of ticks there), 0 for one without tracks"""
    out = []
    for p in range(sh.P):
        if sh.fc[p]:
            out.append((int(rng.integers(0, 3)), None) if for_audit else (0, None))
        elif sh.ft[p]:
            out.append((_pick(rng, (0, 1, "L-1", "L+3")), sh.ft[p]))
        else:
            out.append((0, None))
    return tuple(out)


def _field_columns(rng, sh, chain):
    """the columns of a field coupling that the shadow state accepts: (p, column, q, scale, anchor); column: 0, 1, 'M-1'"""
    P = sh.P
    can = [p for p in range(P) if not sh.ft[p]]
    if not can:
        return None
    if chain and P == 3 and set(can) >= {0, 1}:      # 0 rides on 1 and 2, 1 rides on 2: chained sources
        return ((0, 0, 1, 0, 0), (0, "M-1", 2, 2, 2), (1, 1, 2, 0, 3))
    pops = [p for p in can if rng.integers(0, 2)] or can[:1]
    cols = []
    for p in pops:
        others = [q for q in range(P) if q != p]
        kind = int(rng.integers(0, 3))       # one column, two columns, all three named columns
        for j, c in enumerate((0, "M-1", 1)[:kind + 1]):
            cols.append((p, c, _pick(rng, others), int(rng.integers(0, len(SCALES))), int(rng.integers(0, len(ANCHORS)))))
    return tuple(cols)


def _draw_input(rng, sh, op, attach=False):
    """(op, args) for an input-changing op under the shadow state, which it updates; None where the state leaves no
    accepted call of that kind. attach: an upload, not a detach"""
    P = sh.P
    if op == "set_repulsive_track":
        kind = int(rng.integers(0, 5))
        if kind == 0 or (kind < 3 and any(sh.rep) and sh.rep_src is None):      # (the detach that leaves no track at all)
            sh.rep = [None] * P
            return op, (None,)
        want_long = None
        if kind == 1:                       # a shorter upload after a longer one, and the other way round
            want_long = not sh.last_long
        names = _names(rng, P, want_long=want_long)
        sh.last_long = any(n in ("Lcap", "Lcap+5") for n in names)
        sh.rep = list(names)
        return op, names
    if op == "couple_tracks":
        if rng.integers(0, 4) == 0 or (sh.rep_src is not None and rng.integers(0, 2) == 0):
            sh.rep_src = None
            return op, (None, 0)
        src = [-1] * P
        for p in range(P):
            if rng.integers(0, 3) > 0:
                src[p] = _pick(rng, [q for q in range(P) if q != p])
        if all(q < 0 for q in src):
            src[0] = 1
        sh.rep_src = tuple(src)
        return op, (tuple(src), _pick(rng, (0, 1, "cap")))
    if op == "set_obstacle_tracks":
        if rng.integers(0, 5) == 0 and not attach:
            sh.ft = [None] * P
            return op, (None,)
        if all(sh.fc):
            return None
        want_long = (not sh.last_long) if rng.integers(0, 3) == 0 else None
        names = _names(rng, P, coupled=sh.fc, want_long=want_long)
        sh.last_long = any(n in ("Lcap", "Lcap+5") for n in names)
        sh.ft = list(names)
        return op, names
    if op == "set_obstacle_track_offset":
        if not sh.ft_on():
            return None
        return op, _first_specs(rng, sh)
    if op == "couple_obstacle_tracks":
        if rng.integers(0, 4) == 0:
            sh.fc = [False] * P
            return op, (None, 0)
        cols = _field_columns(rng, sh, chain=bool(rng.integers(0, 2)))
        if cols is None:
            return None
        sh.fc = [any(c[0] == p for c in cols) for p in range(P)]
        return op, (cols, _pick(rng, (0, 1, "cap")))
    if op == "set_initial_position":
        # Once a rollout has run, the next launch comes from a tick: its reset hands every agent the real agent's
        # velocity. A bare pmaf_start there starts from the population's reset state on the device and from each agent's
        # own last velocity in the oracle -- the planner's own boundary, not an order rule of the tracks.
        sh.waiting = False
        sh.restarted = sh.launched
        return op, (int(rng.integers(0, len(DELTAS))),)
    if op == "set_real_position":
        if rng.integers(0, 2) == 0:
            sh.jumped = not sh.jumped
            return op, (len(DELTAS) + (0 if sh.jumped else 1),)
        return op, (int(rng.integers(0, len(DELTAS))),)
    if op == "handover":
        sh.reset()
        return op, ()
    raise AssertionError(op)


def _draw_read(rng, sh, op):
    P = sh.P
    v, m, h = int(rng.integers(0, 3)), int(rng.integers(0, len(MARGINS))), int(rng.integers(0, len(HORIZONS)))
    if op in ("get_repulsive_track", "get_obstacle_tracks"):
        return op, ()
    if not sh.launched:
        return None
    if op == "evaluate_paths":
        return op, (v, m)
    if op == "evaluate_paths_tracked":
        first = _first_specs(rng, sh, True) if sh.ft_on() and rng.integers(0, 3) > 0 else None
        return op, (v, m, first)
    if op == "cross_audit":
        a = int(rng.integers(0, P))
        return op, (a, _pick(rng, [q for q in range(P) if q != a]), int(rng.integers(0, len(SEPARATIONS))))
    if not sh.selected:
        return None
    prev = bool(rng.integers(0, 2))
    if op == "select_clear":
        return op, (v, m, h, prev)
    if op == "select_clear_tracked":
        first = _first_specs(rng, sh, True) if sh.ft_on() and rng.integers(0, 3) > 0 else None
        return op, (v, m, h, prev, bool(rng.integers(0, 2)), first)
    if op == "select_pair_clear":
        a = int(rng.integers(0, P))
        b = _pick(rng, [q for q in range(P) if q != a])
        return op, (a, b, v, m, h, bool(rng.integers(0, 2)), int(rng.integers(0, len(LATES))),
                    int(rng.integers(0, len(SEPARATIONS))), prev)
    raise AssertionError(op)


def _draw_refusal(rng, sh, op):
    """(op, args) where the shadow state makes the contract refuse the call; None elsewhere"""
    P = sh.P
    if op == "refuse_couple_field_on_uploaded":
        up = [p for p in range(P) if sh.ft[p]]
        if not up:
            return None
        p = _pick(rng, up)
        return op, (((p, 0, _pick(rng, [q for q in range(P) if q != p]), 0, 0),), 1)
    if op == "refuse_upload_on_coupled":
        co = [p for p in range(P) if sh.fc[p]]
        if not co:
            return None
        names = [None] * P
        names[_pick(rng, co)] = _pick(rng, LENGTH_NAMES)
        return op, tuple(names)
    if op == "refuse_offset_on_coupled":
        co = [p for p in range(P) if sh.fc[p]]
        if not co:
            return None
        first = [(0, None)] * P
        first[_pick(rng, co)] = (int(rng.integers(1, 4)), None)
        return op, tuple(first)
    if op == "refuse_offset_without_tracks":
        if sh.ft_on():
            return None
        return op, tuple((int(rng.integers(0, 3)), None) for _ in range(P))
    if op == "refuse_couple_self":
        p = int(rng.integers(0, P))
        which = _pick(rng, ("couple_tracks", "couple_obstacle_tracks"))
        return op, (which, p)
    if op == "refuse_couple_range":
        p = int(rng.integers(0, P))
        which = _pick(rng, ("couple_tracks", "couple_obstacle_tracks"))
        return op, (which, p, P + int(rng.integers(0, 2)))
    if op == "refuse_negative_shift":
        return op, (_pick(rng, ("couple_tracks", "couple_obstacle_tracks")), -int(rng.integers(1, 3)))
    raise AssertionError(op)


def _draw_tick(rng, sh):
    if sh.waiting:
        raise AssertionError("a reset waits for its start")
    m, h = int(rng.integers(0, len(MARGINS))), int(rng.integers(1, len(HORIZONS)))
    prev = bool(rng.integers(0, 2)) and sh.selected
    op = _pick(rng, TICK_OPS[:-1])
    if op == "tick":
        args = ()
    elif op in ("tick5", "reset5"):
        args = ()
    elif op == "tick5_adopt_best":
        args = (tuple(_pick(rng, (-1, 1, 2, 3, 4, 5)) for _ in range(sh.P)),)      # per population: -1 keeps, else an offset to the best
    elif op == "tick5_select_clear":
        args = (m, h, prev)
    elif op == "tick5_select_clear_tracked":
        args = (m, h, prev, bool(rng.integers(0, 2)))
    else:
        args = (m, h, prev)
    sh.selected = True
    sh.ticks += 1
    if op == "reset5":
        sh.waiting = True
    else:
        sh.launched = True
    return op, args


def sequence(seed):
    """(shape, P, ops): ops a list of (op, args)"""
    rng = np.random.default_rng(int(seed))
    shape = SHAPES[int(seed) % len(SHAPES)]
    P = 3 if (int(seed) // len(SHAPES)) % 3 == 2 and shape.startswith("M3") else 2
    sh = _Shadow(P)
    ops = []
    n_ticks = int(rng.integers(5, MAX_TICKS))       # (a restart between a reset and its launch adds one)
    refusals = tuple(k for k in REFUSALS if k != "refuse_start_after_stepping")

    def between(n):
        for _ in range(n):
            kind = int(rng.integers(0, 10))
            if kind < 5:
                op = _pick(rng, INPUT_OPS)
                if op == "set_obstacle_track_offset" and not sh.ft_on():
                    ops.append(_draw_input(rng, sh, "set_obstacle_tracks", attach=True))
                got = _draw_input(rng, sh, op)
            elif kind < 8:
                got = _draw_read(rng, sh, _pick(rng, READ_OPS))
            else:
                for _ in range(3):      # (most refusals need a state: an upload, a coupling, neither)
                    got = _draw_refusal(rng, sh, _pick(rng, refusals))
                    if got is not None:
                        break
            if got is not None:
                ops.append(got)

    ops.append(("set_initial_position", (0,)))
    between(int(rng.integers(1, 5)))
    ops.append(("start", ()))
    sh.launched, sh.waiting = True, False
    while sh.ticks < n_ticks:
        between(int(rng.integers(0, 5)))
        if sh.waiting:
            ops.append(("start", ()))
            sh.launched, sh.waiting = True, False
            continue
        if rng.integers(0, 12) == 0:
            # the stepping API in front of a start: refused until the agents are reset, here by the tick that follows
            ops.append(("set_agent_positions", (int(rng.integers(0, len(DELTAS))),)))
            ops.append(("refuse_start_after_stepping", ()))
            sh.restarted = True
        if rng.integers(0, 10) == 0 and not sh.restarted:
            ops.append(("start", ()))       # nothing was reset since the last launch: launches nothing
            continue
        ops.append(_draw_tick(rng, sh))
        sh.restarted = False
        if sh.waiting and sh.rep_src is not None and rng.integers(0, 2) == 0:
            # an upload between the reset, which took the coupled populations' tracks, and the launch that follows them
            ops.append(_draw_input(rng, sh, "set_repulsive_track"))
        if sh.waiting and rng.integers(0, 3) == 0:
            # the paths restart between the reset and the launch: what the reset took is discarded, the fused tick takes anew
            ops.append(_draw_input(rng, sh, "set_initial_position"))
            ops.append(("tick", ()))
            sh.ticks += 1
            sh.restarted = False
    if sh.waiting:
        ops.append(("start", ()))
    between(int(rng.integers(0, 3)))
    return shape, P, ops


# ---- resolving the arguments ------------------------------------------------------------------------------------------
_CONTEXTS = {}


class Context:
    """scenes, lists and named tracks of one (shape, P): computed once per evaluation order, shared, never modified"""

    def __init__(self, orc, scenes, shape, P):
        self.shape, self.P = shape, P
        self.scs = cref.dual_scenes(scenes, shape, moving=True) if P == 2 else cref.triple_scenes(scenes, shape)
        self.env = sref.SHAPES[shape].get("env", {})
        sc0 = self.scs[0]
        self.M = len(sc0["obstacles"]) - 1
        self.cap = int(sc0["max_prediction_steps"])
        self.dt, self.gains, self.ws = sc0["dt"], sc0["cost_gains"], sc0["ws_limits"]
        self.starts = np.stack([s["start"] for s in self.scs])
        self.live = np.stack([s["obstacles"] for s in self.scs])
        self.lists = []
        for v in range(3):      # what the read-only calls are handed: never the ticks' list
            o = self.live.copy()
            o[:, :-1, 0:3] += 0.01 * (v + 1) * np.array([1.0, -1.0, 0.5])
            o[:, -1, 0:3] += 0.005 * v
            self.lists.append(o)
        self.rep, self.ft = [], []
        for sc in self.scs:
            ora = orc.OraclePlanner(sc, mgr_init_pos=sc["start"])
            ora.set_initial_position(sc["start"])
            ora.rollout()
            paths, n = ora.paths()
            self.rep.append(sref.tracks_for(sc, paths[0], int(n[0])))
            self.ft.append(fref.tracks_for(sc, paths[0], int(n[0])))
            ora.close()

    def shift(self, s):
        return self.cap if s == "cap" else int(s)

    def column(self, c):
        return self.M - 1 if c == "M-1" else int(c)

    def first(self, specs):
        out = []
        for p, (f, name) in enumerate(specs):
            if isinstance(f, str):
                f = fref.resolve_first(f, len(self.ft[p][name]))
            out.append(int(f))
        return out

    def attach(self, cols):
        return cref.attach(self.P, self.M, {(p, self.column(c)): (q, SCALES[s], np.array(ANCHORS[a])) for p, c, q, s, a in cols})


def context(orc, scenes, shape, P):
    key = (shape, P, orc.eval_order())
    if key not in _CONTEXTS:
        _CONTEXTS[key] = Context(orc, scenes, shape, P)
    return _CONTEXTS[key]


# ---- one op on one handle ---------------------------------------------------------------------------------------------
class Side:
    """a handle and what later ops derive from its earlier results"""

    def __init__(self, factory):
        self.factory = factory
        self.h = factory()
        self.pick = None

    def close(self):
        self.h.close()


def _refused(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except Exception as e:       # PmafError and ModelError: both carry the contract's code
        code = getattr(e, "code", None)
        if code is None:
            raise
        return ("refused", int(code))
    return ("accepted", 0)


def _five_calls(side, ctx, adopt=None, start=True):
    h = side.h
    h.stop()
    best = np.asarray(h.evaluate(ctx.gains, ctx.ws)).copy()
    ids, sel = best, None
    if adopt is not None:
        ids, sel = adopt(best)
    h.move_real(ctx.live, ctx.dt, 1, ids)
    pos, vel, _ = h.real_state()
    h.reset_agents(pos, vel, ctx.live)
    if start:
        h.start()
    side.pick = np.asarray(ids).copy()
    return {"best": best, "ids": np.asarray(ids), "sel": sel}


def apply(side, ctx, op, args):
    """run one op; returns what the call returned (a refusal: ('refused', code))"""
    h = side.h
    prev_of = lambda use: side.pick if use and side.pick is not None else None
    if op == "start":
        return h.start()
    if op == "tick":
        best = np.asarray(h.tick(ctx.live, ctx.dt, ctx.gains, ctx.ws)).copy()
        side.pick = best
        return best
    if op == "tick5":
        return _five_calls(side, ctx)
    if op == "reset5":
        return _five_calls(side, ctx, start=False)
    if op == "tick5_adopt_best":
        def adopt(best):
            idx = np.array([-1 if k < 0 else (int(b) + k) % ctx_N(h) for b, k in zip(best, args[0])], dtype=np.int32)
            h.adopt_best(idx)
            return np.where(idx >= 0, idx, best).astype(np.int32), None
        return _five_calls(side, ctx, adopt)
    if op == "tick5_select_clear":
        m, hz, use = args
        def adopt(best):
            sel = h.select_clear(ctx.live, MARGINS[m], HORIZONS[hz], prev=prev_of(use), adopt=True)
            return np.asarray(sel["pick"], dtype=np.int32), sel
        return _five_calls(side, ctx, adopt)
    if op == "tick5_select_clear_tracked":
        m, hz, use, skip = args
        def adopt(best):
            sel = h.select_clear_tracked(ctx.live, MARGINS[m], HORIZONS[hz], prev=prev_of(use), adopt=True, skip_trailing=skip)
            return np.asarray(sel["pick"], dtype=np.int32), sel
        return _five_calls(side, ctx, adopt)
    if op in ("audited_tick", "audited_tick_tracked"):
        m, hz, use = args
        out = h.audited_tick(ctx.live, ctx.dt, ctx.gains, ctx.ws, MARGINS[m], HORIZONS[hz], prev=prev_of(use),
                             tracked=op.endswith("tracked"))
        side.pick = np.asarray(out["pick"], dtype=np.int32).copy()
        return out
    if op == "set_repulsive_track":
        return h.set_repulsive_track(None if args == (None,) else [None if n is None else ctx.rep[p][n] for p, n in enumerate(args)])
    if op == "couple_tracks":
        return h.couple_tracks(None if args[0] is None else list(args[0]), ctx.shift(args[1]))
    if op == "set_obstacle_tracks":
        return h.set_obstacle_tracks(None if args == (None,) else [None if n is None else ctx.ft[p][n] for p, n in enumerate(args)])
    if op == "set_obstacle_track_offset":
        return h.set_obstacle_track_offset(ctx.first(args))
    if op == "couple_obstacle_tracks":
        if args[0] is None:
            return h.couple_obstacle_tracks(None)
        return h.couple_obstacle_tracks(*ctx.attach(args[0]), ctx.shift(args[1]))
    if op == "set_initial_position":
        return h.set_initial_position(ctx.starts + np.array(DELTAS[args[0]]))
    if op == "set_real_position":
        return h.set_real_position(np.asarray(h.real_state()[0]).reshape(ctx.P, 3) + np.array((DELTAS + JUMPS)[args[0]]))
    if op == "set_agent_positions":
        return h.set_agent_positions(ctx.starts + np.array(DELTAS[args[0]]))
    if op == "handover":
        blob = h.save_state()
        h.close()
        side.h = side.factory()
        side.h.load_state(blob)
        return None
    if op == "get_repulsive_track":
        return h.get_repulsive_track()
    if op == "get_obstacle_tracks":
        return h.get_obstacle_tracks()
    if op == "evaluate_paths":
        return h.evaluate_paths(ctx.lists[args[0]], MARGINS[args[1]], per_obstacle=True)
    if op == "evaluate_paths_tracked":
        v, m, first = args
        return h.evaluate_paths_tracked(ctx.lists[v], MARGINS[m], per_obstacle=True, first=None if first is None else ctx.first(first))
    if op == "cross_audit":
        return h.cross_audit(args[0], args[1], SEPARATIONS[args[2]], step=True)
    if op == "select_clear":
        v, m, hz, use = args
        return h.select_clear(ctx.lists[v], MARGINS[m], HORIZONS[hz], prev=prev_of(use), adopt=False)
    if op == "select_clear_tracked":
        v, m, hz, use, skip, first = args
        return h.select_clear_tracked(ctx.lists[v], MARGINS[m], HORIZONS[hz], prev=prev_of(use), adopt=False,
                                      first=None if first is None else ctx.first(first), skip_trailing=skip)
    if op == "select_pair_clear":
        a, b, v, m, hz, skip, late, sep, use = args
        pv = None if not use or side.pick is None else (int(side.pick[a]), int(side.pick[b]))
        return h.select_pair_clear(a, b, ctx.lists[v], MARGINS[m], HORIZONS[hz], SEPARATIONS[sep], 0.02, skip_trailing=skip,
                                   late=LATES[late], prev_pair=pv, adopt=False)
    if op == "refuse_couple_field_on_uploaded":
        return _refused(h.couple_obstacle_tracks, *ctx.attach(args[0]), ctx.shift(args[1]))
    if op == "refuse_upload_on_coupled":
        return _refused(h.set_obstacle_tracks, [None if n is None else ctx.ft[p][n] for p, n in enumerate(args)])
    if op in ("refuse_offset_on_coupled", "refuse_offset_without_tracks"):
        return _refused(h.set_obstacle_track_offset, ctx.first(args))
    if op in ("refuse_couple_self", "refuse_couple_range", "refuse_negative_shift"):
        which = args[0]
        shift = args[1] if op == "refuse_negative_shift" else 1
        if op == "refuse_negative_shift":
            p, q = 0, 1
        else:
            p, q = args[1], (args[1] if op == "refuse_couple_self" else args[2])
        if which == "couple_tracks":
            src = [-1] * ctx.P
            src[p] = q
            return _refused(h.couple_tracks, src, shift)
        src = np.full((ctx.P, ctx.M), -1)
        src[p, 0] = q
        return _refused(h.couple_obstacle_tracks, src, 1.0, np.zeros(3), shift)
    if op == "refuse_start_after_stepping":
        return _refused(h.start)
    raise AssertionError(op)


def ctx_N(h):
    return int(h.N)


def observe(h):
    """every observable the comparison looks at after an op that can change state (the getters wait for a running
    rollout)"""
    paths, n = h.paths()
    return {"paths": paths, "n_points": n, "costs": h.costs(), "rot_vecs": h.rot_vecs(), "known": h.known(),
            "min_obs_dist": h.min_obs_dist(), "success": h.success(), "agent_vel": h.agent_vel(), "real_state": h.real_state(),
            "best": h.best(), "get_repulsive_track": h.get_repulsive_track(), "get_obstacle_tracks": h.get_obstacle_tracks()}


def flatten(value, name):
    """(field, array) leaves of a returned value: dicts by key, tuples and lists by index"""
    if isinstance(value, dict):
        for k in sorted(value):
            yield from flatten(value[k], "%s.%s" % (name, k))
    elif isinstance(value, (tuple, list)) and not all(isinstance(v, (int, float, bool, np.integer, np.floating)) for v in value):
        for j, v in enumerate(value):
            yield from flatten(v, "%s[%d]" % (name, j))
    elif value is None:
        yield name, np.zeros(0)
    else:
        yield name, np.asarray(value)


def trace(seed, ctx, ops, factory):
    """run the sequence on a handle of `factory`'s; yields (op index, op, field, array) for the op's own return value and,
    after an op that can change state, for every observable. Closes the handle at the end."""
    side = Side(factory)
    try:
        for i, (op, args) in enumerate(ops):
            ret = apply(side, ctx, op, args)
            if op in REFUSALS:
                yield i, op, "return.code", np.asarray(ret[1] if ret[0] == "refused" else 0)
            else:
                for field, a in flatten(ret, "return"):
                    yield i, op, field, a
            if op not in READ_OPS:
                for field, a in flatten(observe(side.h), "state"):
                    yield i, op, field, a
    finally:
        side.close()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        a, b = np.squeeze(a), np.squeeze(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f")


def first_mismatch(seed, got, want):
    """compare two traces item by item: None, or (seed, op index, op, field, got, want) of the first difference"""
    for g, w in zip(got, want):
        if g[:3] != w[:3]:
            return (seed, g[0], g[1], "trace shape: %s / %s" % (g[2], w[2]), None, None)
        if not same(g[3], w[3]):
            return (seed, g[0], g[1], g[2], g[3], w[3])
    return None


def describe(mismatch):
    seed, i, op, field, got, want = mismatch
    return "seed %d op %d (%s) field %s:\n got %r\nwant %r" % (seed, i, op, field, got, want)


# The smallest prefix of 0, 1, 2, ... whose sequences meet the four conditions tests/test_sequence_model.py asserts.
SEEDS = tuple(range(44))
