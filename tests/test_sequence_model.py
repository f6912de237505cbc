"""The composed model of tests/sequence_model.py and the seeded sequences of tests/sequence_cases.py without a device.
The model is no new truth: it reproduces the per-feature modules' own scripted tick sequences bit for bit, and what it
returns for an audit or a selection is what the per-feature references give on those paths. The committed SEEDS are the
smallest prefix of 0, 1, 2, ... under which (a) every op of the alphabet occurs in at least three sequences and on at
least two shapes, (b) every ordered pair of input-changing ops occurs with no tick between the two and with at least one,
(c) every refusal occurs at least twice, and (d) every mutant of the model changes a compared value in at least two
sequences -- measured through the comparison tests/test_sequence_gpu.py runs against the device, so what is measured is
that comparison's reach."""
import numpy as np
import pytest

import field_couple_reference as cref
import field_track_reference as fref
import path_audit_reference as par
import select_clear_reference as scr
import sentinel_track_reference as sref
import sequence_cases as cases
import sequence_model as model
import tracked_audit_reference as tar

RES_KEYS = ("paths", "n_points", "min_obs", "known", "rot", "vel")


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


def results(m, p):
    paths, n = m.paths()
    return dict(paths=paths[p], n_points=n[p], min_obs=m.min_obs_dist()[p], known=m.known()[p], rot=m.rot_vecs()[p],
                vel=m.agent_vel()[p])


def same(got, want, tag):
    for k in RES_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (tag, k))


def five_calls(m, sc, live, between=None):
    m.stop()
    best = m.evaluate(sc["cost_gains"], sc["ws_limits"])
    m.move_real(live, sc["dt"], 1, best)
    pos, vel, _ = m.real_state()
    m.reset_agents(pos, vel, live)
    if between is not None:
        between()
    m.start()
    return best


# ---- the model against the per-feature modules' own sequences ---------------------------------------------------------------
@pytest.mark.parametrize("shape,name", [("M3-cap70-moving", "sweep"), ("M59-cap9-general-moving", "short")])
def test_model_reproduces_tracked_ticks(oracle, scenes, shape, name):
    """field_track_reference.tracked_ticks: uploaded obstacle tracks, the offset one point further every tick"""
    sc = sref.build_scene(scenes, shape)
    ora = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
    ora.set_initial_position(sc["start"])
    ora.rollout()
    paths, n = ora.paths()
    ft = fref.tracks_for(sc, paths[0], int(n[0]))[name]
    first, ticks = fref.tracked_ticks(oracle, sc, ft, 4)
    untracked, _ = fref.tracked_ticks(oracle, sc, None, 0)
    assert not np.array_equal(first["paths"], untracked["paths"])
    live = sc["obstacles"][None]
    m = model.ModelHandle(oracle, [sc])
    m.set_initial_position(sc["start"])
    m.set_obstacle_tracks([ft])
    m.start()
    same(results(m, 0), first, "first rollout")
    np.testing.assert_array_equal(m.success()[0], first["reached"])
    for t, (best, res) in enumerate(ticks):
        b = five_calls(m, sc, live, lambda: m.set_obstacle_track_offset([t + 1]))
        assert int(b[0]) == best, t
        same(results(m, 0), res, "tick %d" % t)
        used, off = m.get_obstacle_tracks()
        np.testing.assert_array_equal(used[0], ft)
        assert list(off) == [t + 1]


@pytest.mark.parametrize("shift", [0, 1])
def test_model_reproduces_coupled_ticks(oracle, scenes, shift):
    """sentinel_track_reference.coupled_ticks: two arms on each other's selected paths, fused and five-call ticks in turn"""
    scs = sref.dual_scenes(scenes)
    first, ticks = sref.coupled_ticks(oracle, scs, [1, 0], shift, 4)
    live = np.stack([s["obstacles"] for s in scs])
    m = model.ModelHandle(oracle, scs)
    m.set_initial_position(np.stack([s["start"] for s in scs]))
    m.couple_tracks([1, 0], shift)
    m.start()
    for p in range(2):
        same(results(m, p), first[p], "first rollout pop %d" % p)
    assert [len(t) for t in m.get_repulsive_track()] == [0, 0]
    for t, (best, tracks, res) in enumerate(ticks):
        if t % 2:
            b = five_calls(m, scs[0], live)
        else:
            b = m.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
        assert list(b) == list(best), t
        used = m.get_repulsive_track()
        for p in range(2):
            np.testing.assert_array_equal(used[p], tracks[p], err_msg="tick %d pop %d track" % (t, p))
            same(results(m, p), res[p], "tick %d pop %d" % (t, p))


@pytest.mark.parametrize("repulsive", [None, (1, 0)], ids=["field", "field+repulsive"])
def test_model_reproduces_field_coupled_ticks_and_the_audits_on_their_paths(oracle, scenes, repulsive):
    """field_couple_reference.field_coupled_ticks with and without repulsive_src; then every audit and selection of the
    model on the paths that sequence produced against the reference it dispatches to, fed by hand"""
    shape, short, shift = cref.GROUP_CASES["plain-dpp"][0]
    scs = cref.dual_scenes(scenes, shape, short, moving=True)
    src, scale, anchor = cref.dual_attach(len(scs[0]["obstacles"]) - 1)
    first, ticks = cref.field_coupled_ticks(oracle, scs, src, scale, anchor, shift, 4, repulsive_src=repulsive)
    live = np.stack([s["obstacles"] for s in scs])
    sc = scs[0]
    m = model.ModelHandle(oracle, scs)
    m.set_initial_position(np.stack([s["start"] for s in scs]))
    m.couple_obstacle_tracks(src, scale, anchor, shift)
    if repulsive is not None:
        m.couple_tracks(list(repulsive), shift)
    m.start()
    for p in range(2):
        same(results(m, p), first[p], "first rollout pop %d" % p)
    for t, (best, tracks, res) in enumerate(ticks):
        if t % 2:
            b = five_calls(m, sc, live)
        else:
            b = m.tick(live, sc["dt"], sc["cost_gains"], sc["ws_limits"])
        assert list(b) == list(best), t
        used, off = m.get_obstacle_tracks()
        assert list(off) == [0, 0]
        for p in range(2):
            np.testing.assert_array_equal(used[p], tracks[p], err_msg="tick %d pop %d composed tracks" % (t, p))
            same(results(m, p), res[p], "tick %d pop %d" % (t, p))
    # the audits and selections on these paths: the references, fed by hand with what the sequence produced
    m.evaluate(sc["cost_gains"], sc["ws_limits"])
    order = oracle.eval_order()
    res, tracks = ticks[-1][2], [t.tolist() for t in ticks[-1][1]]
    paths, n = [r["paths"].tolist() for r in res], [r["n_points"].tolist() for r in res]
    costs = m.costs().tolist()
    lst, dt, rad = live.tolist(), sc["dt"], sc["radius"]

    def check(got, want, tag):
        for k in got:
            np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg="%s %s" % (tag, k))

    check(m.evaluate_paths(live, 0.02, per_obstacle=True), par.audit(paths, n, lst, dt, rad, 0.02, order), "evaluate_paths")
    check(m.select_clear(live, 0.02, 30, prev=[1, 1]), scr.select_clear(paths, n, lst, costs, dt, rad, 0.02, 30, order, [1, 1]),
          "select_clear")
    for f in ([1, 1], [0, 3]):
        check(m.evaluate_paths_tracked(live, 0.02, per_obstacle=True, first=f),
              tar.audit(paths, n, lst, tracks, f, dt, rad, 0.02, order), "evaluate_paths_tracked %r" % f)
        for skip in (False, True):
            check(m.select_clear_tracked(live, 0.02, 30, prev=[1, 1], first=f, skip_trailing=skip),
                  tar.select_clear(paths, n, lst, tracks, f, costs, dt, rad, 0.02, 30, skip, order, [1, 1]),
                  "select_clear_tracked %r %r" % (f, skip))
    tracked = m.evaluate_paths_tracked(live, 0.02, first=[1, 1])
    assert not np.array_equal(tracked["clearance"], m.evaluate_paths(live, 0.02)["clearance"])


# ---- the committed seeds ------------------------------------------------------------------------------------------------------
_BASE = {}


def make(oracle, ctx, mutant=None):
    return lambda: model.ModelHandle(oracle, ctx.scs, mutant=mutant)


def base_trace(oracle, scenes, seed):
    """the model's own trace of one seed: computed once per evaluation order, shared, never modified"""
    key = (seed, oracle.eval_order())
    if key not in _BASE:
        shape, P, ops = cases.sequence(seed)
        ctx = cases.context(oracle, scenes, shape, P)
        _BASE[key] = (ctx, ops, list(cases.trace(seed, ctx, ops, make(oracle, ctx))))
    return _BASE[key]


def op_coverage(seeds):
    """op -> (the seeds whose sequence has it, the shapes of those)"""
    cov = {op: (set(), set()) for op in cases.ALPHABET}
    for s in seeds:
        shape, _, ops = cases.sequence(s)
        for op, _ in ops:
            cov[op][0].add(s)
            cov[op][1].add(shape)
    return cov


def pair_coverage(seeds):
    """(near, far): the ordered pairs of input-changing ops with no tick between the two / with at least one"""
    near, far = set(), set()
    for s in seeds:
        ops = [op for op, _ in cases.sequence(s)[2]]
        for i, a in enumerate(ops):
            if a not in cases.INPUT_OPS:
                continue
            ticked = False
            for b in ops[i + 1:]:
                if b in cases.TICK_OPS:
                    ticked = True
                elif b in cases.INPUT_OPS:
                    (far if ticked else near).add((a, b))
    return near, far


def refusal_counts(seeds):
    n = {r: 0 for r in cases.REFUSALS}
    for s in seeds:
        for op, _ in cases.sequence(s)[2]:
            if op in n:
                n[op] += 1
    return n


_CAUGHT = {}
_COUPLINGS = ("couple_tracks", "couple_obstacle_tracks")
_ADOPTING = ("tick5_adopt_best", "tick5_select_clear", "tick5_select_clear_tracked", "audited_tick", "audited_tick_tracked")
# the calls through which alone a mutant's broken rule can be reached: a sequence without any of them is not run
REACHED_THROUGH = {
    "detach_keeps_length": ("set_repulsive_track", "couple_tracks"),
    "upload_keeps_offset": ("set_obstacle_track_offset",),
    "upload_wins_over_coupling": ("couple_tracks",),
    "take_at_launch_in_five_call": _COUPLINGS,
    "take_before_adopt": _COUPLINGS,
    "set_initial_keeps_taken": _COUPLINGS,
    "getter_reads_attached": _COUPLINGS,
    "coupled_audit_reads_next": ("couple_obstacle_tracks",),
    "grow_drops_neighbour": ("couple_obstacle_tracks",),
    "blob_carries_tracks": ("handover",),
    "audit_moves_offset": ("evaluate_paths_tracked", "select_clear_tracked"),
    "adopt_ignored_by_real_step": _ADOPTING,
    "upload_drops_taken": ("couple_tracks",),
}


def caught(oracle, scenes, seed, mutant):
    """(op index, op, field) of the first value the comparison sees change when the model with `mutant` runs this seed's
    sequence against the model without, or None"""
    key = (seed, mutant, oracle.eval_order())
    if key not in _CAUGHT:
        ctx, ops, base = base_trace(oracle, scenes, seed)
        if not {op for op, _ in ops}.intersection(REACHED_THROUGH[mutant]):
            _CAUGHT[key] = None
        else:
            got = cases.trace(seed, ctx, ops, make(oracle, ctx, mutant))
            try:
                bad = cases.first_mismatch(seed, got, iter(base))
            finally:
                got.close()
            _CAUGHT[key] = None if bad is None else bad[1:4]
    return _CAUGHT[key]


def first_two(oracle, scenes, seeds, mutant):
    """the first two seeds whose sequence tells the mutant from the model (fewer: there are no two)"""
    hits = []
    for s in seeds:
        if caught(oracle, scenes, s, mutant) is not None:
            hits.append(s)
            if len(hits) == 2:
                break
    return hits


def unmet(oracle, scenes, seeds, static_only=False):
    """what of (a) ... (d) the seeds do not meet: a list of strings, empty when all four hold"""
    out = []
    for op, (in_seeds, on_shapes) in op_coverage(seeds).items():
        if len(in_seeds) < 3 or len(on_shapes) < 2:
            out.append("(a) %s: %d sequences, %d shapes" % (op, len(in_seeds), len(on_shapes)))
    near, far = pair_coverage(seeds)
    for a in cases.INPUT_OPS:
        for b in cases.INPUT_OPS:
            if (a, b) not in near:
                out.append("(b) %s -> %s: never without a tick between" % (a, b))
            if (a, b) not in far:
                out.append("(b) %s -> %s: never with a tick between" % (a, b))
    for r, n in refusal_counts(seeds).items():
        if n < 2:
            out.append("(c) %s: %d times" % (r, n))
    if static_only:
        return out
    for mutant in model.MUTANTS:
        hits = first_two(oracle, scenes, seeds, mutant)
        if len(hits) < 2:
            out.append("(d) %s: changes a compared value in %d sequences %r" % (mutant, len(hits), hits))
    return out


def test_seeds_meet_the_four_conditions_and_no_shorter_prefix_does(oracle, scenes):
    assert cases.SEEDS == tuple(range(len(cases.SEEDS)))
    missing = unmet(oracle, scenes, cases.SEEDS)
    assert not missing, "\n".join(missing)
    assert unmet(oracle, scenes, cases.SEEDS[:-1]), "SEEDS is not the smallest prefix that meets the conditions"
    for mutant in model.MUTANTS:
        print(mutant, {s: caught(oracle, scenes, s, mutant) for s in first_two(oracle, scenes, cases.SEEDS, mutant)})


def test_sequences_are_reproducible_and_within_their_bounds():
    for s in cases.SEEDS:
        a, b = cases.sequence(s), cases.sequence(s)
        assert a == b and repr(a) == repr(b), s
        shape, P, ops = a
        assert shape in cases.SHAPES and P in (2, 3)
        assert sum(1 for op, _ in ops if op in cases.TICK_OPS and op != "start") <= cases.MAX_TICKS
        assert all(op in cases.ALPHABET for op, _ in ops)


def test_a_refused_call_carries_the_contracts_code_and_leaves_the_model_unchanged(oracle, scenes):
    seen = 0
    for s in cases.SEEDS:
        _, ops, tr = base_trace(oracle, scenes, s)
        state = {}       # op index -> {field: array}
        for i, op, field, a in tr:
            if field.startswith("state."):
                state.setdefault(i, {})[field] = a
            elif op in cases.REFUSALS:
                assert field == "return.code" and int(a) == cases.REFUSALS[op], (s, i, op, a)
        for i, (op, _) in enumerate(ops):
            if op not in cases.REFUSALS:
                continue
            before = max(j for j in state if j < i)
            assert state[i].keys() == state[before].keys()
            for field in state[i]:
                assert cases.same(state[i][field], state[before][field]), (s, i, op, field)
            seen += 1
    assert seen >= 2 * len(cases.REFUSALS)
