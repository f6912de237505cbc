"""The obstacle tracks' device-side source on the GPU (pmaf_couple_obstacle_tracks; k_fcouple_take / k_fcouple_compose of
csrc/pmaf_k_fcouple.hip) through the C-ABI, at tolerance 0: the composed tracks (pmaf_get_obstacle_tracks) against
compose_tracks and the coupled tick sequences against field_coupled_ticks, both of tests/field_couple_reference.py.
tests/test_field_couple.py validates the reference on the CPU and shows which rule each case is sensitive to. The
references take the evaluation order from the oracle / pmaf_eval_order(), so the file passes unchanged under
PMAF_VARIANT=rassoc."""
import numpy as np
import pytest

import field_couple_reference as cref
import field_track_reference as fref
import sentinel_track_reference as sref
import tracked_audit_reference as tar

pytestmark = pytest.mark.gpu

KEYS = ("paths", "n_points", "min_obs", "known", "rot", "vel", "reached", "costs")
TICK_KEYS = ("paths", "n_points", "min_obs", "known", "rot", "vel")
ERR_INVALID, ERR_STATE = -1, -3


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("PMAF_SUM", "PMAF_FORCE_GENERIC", "PMAF_PLAIN_STEP", "PMAF_MW", "PMAF_W64_SLICE"):
        monkeypatch.delenv(k, raising=False)


def planner(pmaf, monkeypatch, scs, shape=None, **kw):
    for k, v in (sref.SHAPES[shape].get("env", {}) if shape else {}).items():
        monkeypatch.setenv(k, v)
    scs = scs if isinstance(scs, list) else [scs]
    pl = pmaf.PmafPlanner(scs if len(scs) > 1 else scs[0], device=0, mgr_init_pos=np.stack([s["start"] for s in scs]), **kw)
    pl.set_initial_position(np.stack([s["start"] for s in scs]))
    return pl


def state(pl):
    pl.stop()
    paths, n = pl.paths()
    return dict(paths=paths, n_points=n, min_obs=pl.min_obs_dist(), known=pl.known(), rot=pl.rot_vecs(), vel=pl.agent_vel(),
                reached=pl.success())


def same(got, want, p, tag, keys=TICK_KEYS, latched_only=False):
    g = {k: np.asarray(got[k][p]) for k in keys}
    w = {k: np.asarray(want[k]) for k in keys}
    if latched_only:      # (rotation vectors of obstacles THIS rollout did not latch are left over from earlier ones)
        g["rot"] = g["rot"] * g["known"][..., None]
        w["rot"] = w["rot"] * w["known"][..., None]
    for k in keys:
        print("%s pop %d %s: %d differing entries" % (tag, p, k, int((g[k] != w[k]).sum())))
    for k in keys:
        np.testing.assert_array_equal(g[k], w[k], err_msg="%s pop %d %s" % (tag, p, k))


def same_bits(got, want, what):
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float64))
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    print("%s: %d of %d values differ" % (what, int(bad.sum()), bad.size))
    assert not bad.any(), "%s: first at %s: %r != %r" % (what, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def expected_tracks(scs, paths, n, pick, src, scale, anchor, shift, lists=None, has_best=None, mutant=None):
    """compose_tracks for every population from the paths as they lay in front of the selection's rollout"""
    P = len(scs)
    sel_p = [np.asarray(paths[q][int(pick[q])]) for q in range(P)]
    sel_n = [int(n[q][int(pick[q])]) for q in range(P)]
    hb = [True] * P if has_best is None else has_best
    return [cref.compose_tracks(sel_p, sel_n, hb, src[p], scale[p], anchor[p], shift,
                                scs[p]["obstacles"] if lists is None else lists[p], scs[p]["dt"],
                                scs[p]["max_prediction_steps"], mutant) for p in range(P)]


def check_getter(pl, want, tag):
    used, first = pl.get_obstacle_tracks()
    assert list(first) == [0] * len(want), tag
    for p, w in enumerate(want):
        assert used[p].shape == w.shape, (tag, p, used[p].shape, w.shape)
        same_bits(used[p], w, "%s pop %d composed tracks" % (tag, p))


# ---- the composed tracks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,shift", [("M3-cap70", 0), ("M3-cap70", 1), ("M3-cap70", 500), ("M3-cap9", 1), ("M59-cap70-moving", 2),
                                         ("M60-cap70-lds-general-moving", 1), ("M59-cap9-general-moving", 0)], ids=str)
def test_getter_equals_the_composition(pmaf, oracle, scenes, monkeypatch, shape, shift):
    """pmaf_get_obstacle_tracks after a launch: positions, velocities, len = cap, first = 0, bit for bit -- on
    field_couple_reference.fast_scenes, where the reciprocal multiply differs from the division in some velocities
    (asserted for the 70-point shapes). shift >= n: one held point, every velocity +0.0. Before any selection: len 0."""
    scs = cref.fast_scenes(scenes, shape)
    M, cap = len(scs[0]["obstacles"]) - 1, scs[0]["max_prediction_steps"]
    src, scale, anchor = cref.dual_attach(M)
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs, shape)
    try:
        pl.couple_obstacle_tracks(src, scale, anchor, shift)
        used, first = pl.get_obstacle_tracks()
        assert [len(t) for t in used] == [0, 0] and list(first) == [0, 0]
        n0 = pl.launch_count()
        pl.start()
        pl.stop()
        assert pl.launch_count() == n0 + 1
        used, first = pl.get_obstacle_tracks()
        assert [len(t) for t in used] == [0, 0] and list(first) == [0, 0]      # no selection yet
        recip_seen = False
        for t in range(2):
            paths, n = pl.paths()
            b = pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            pl.stop()
            want = expected_tracks(scs, paths, n, b, src, scale, anchor, shift)
            assert all(w.shape == (cap, M, 6) for w in want)
            check_getter(pl, want, "%s shift %d tick %d" % (shape, shift, t))
            if shift >= cap:
                for w in want:
                    assert not np.any(w[:, [0, M - 1], 3:6]) and (w[:, 0, 0:3] == w[0, 0, 0:3]).all()
            mut = expected_tracks(scs, paths, n, b, src, scale, anchor, shift, mutant="recip")
            recip_seen = recip_seen or any(not np.array_equal(a, c) for a, c in zip(mut, want))
        if cap == 70 and shift < cap:
            assert recip_seen, "no component of this case tells d * (1 / dt) from the division"
    finally:
        pl.close()


# ---- tick sequences -------------------------------------------------------------------------------------------------------
_TICKS = {}


def reference_ticks(oracle, scenes, shape, short, shift, **kw):
    """(scenes, coupling, first rollouts, ticks) of one case: computed once, shared, never modified"""
    key = (shape, short, shift, tuple(sorted(kw.items())), oracle.eval_order())
    if key not in _TICKS:
        scs = cref.dual_scenes(scenes, shape, short, moving=True)
        att = cref.dual_attach(len(scs[0]["obstacles"]) - 1)
        first, ticks = cref.field_coupled_ticks(oracle, scs, att[0], att[1], att[2], shift, 6, **kw)
        _TICKS[key] = (scs, att, first, ticks)
    return _TICKS[key]


def one_tick(pl, scs, live, style, adopt=None):
    if style == "tick":
        return pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
    pl.stop()
    b = pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
    if adopt is not None:
        b = np.asarray(adopt, dtype=np.int32)
        pl.adopt_best(b)
    pl.move_real(live, scs[0]["dt"], 1, b)
    pos, vel, _ = pl.real_state()
    pl.reset_agents(pos, vel, live)
    pl.start()
    return b


CASES = [(g,) + c for g, cs in cref.GROUP_CASES.items() for c in cs]


@pytest.mark.parametrize("style", ["tick", "calls"])
@pytest.mark.parametrize("group,shape,short,shift", CASES, ids=str)
def test_coupled_ticks(pmaf, oracle, scenes, monkeypatch, group, shape, short, shift, style):
    """six ticks of two arms whose columns 0 and M - 1 ride on each other's selected paths -- the fused pmaf_tick, or the
    node's five calls, whose reset cuts the paths before the rollout is launched (the take happens at the reset) --
    against the composer: the same reference, so both styles give the same bits. The first rollout, before any
    selection, runs untracked. `short`: the source path ends after a few points (the hold, the zero velocity, unattached
    columns that move on to cap); column 0 enters the detection shell mid-rollout (tests/test_field_couple.py)."""
    scs, (src, scale, anchor), first, ticks = reference_ticks(oracle, scenes, shape, short, shift)
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs, shape)
    try:
        cfg = pl.launch_config()
        assert cfg["lanes_per_agent"] == 64 and cfg["waves_per_agent"] == 1 and not cfg["priority_slices"]
        pl.couple_obstacle_tracks(src, scale, anchor, shift)
        pl.start()
        got = state(pl)
        for p in range(2):
            same(got, first[p], p, "first rollout")
        for t, (best, tracks, res) in enumerate(ticks):
            n0 = pl.launch_count()
            b = one_tick(pl, scs, live, style)
            got = state(pl)
            assert pl.launch_count() == n0 + 1
            assert list(b) == list(best), t
            check_getter(pl, tracks, "tick %d" % t)
            for p in range(2):
                same(got, res[p], p, "%s tick %d" % (style, t))
    finally:
        pl.close()


def test_three_populations_two_sources_of_different_length(pmaf, oracle, scenes, monkeypatch):
    """P = 3: columns 0 and M - 1 of population 0 follow populations 1 and 2, whose selected paths have different lengths
    (population 2's goal is 0.13 m away); population 1 follows population 2 with one column; population 2 is uncoupled"""
    shape = "M3-cap70"
    scs = cref.triple_scenes(scenes, shape)
    M = 3
    src, scale, anchor = cref.attach(3, M, {(0, 0): (1, 1.0, cref.SIDE), (0, M - 1): (2, 0.9, np.array([-0.03, 0.02, 0.0])),
                                            (1, 1): (2, 1.0, np.array([0.0, 0.75, 0.05]))})
    first, ticks = cref.field_coupled_ticks(oracle, scs, src, scale, anchor, 1, 3)
    assert ticks[1][1][2].shape == (0, M, 6)
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs)
    try:
        pl.couple_obstacle_tracks(src, scale, anchor, 1)
        pl.start()
        got = state(pl)
        for p in range(3):
            same(got, first[p], p, "first rollout")
        lens = set()
        for t, (best, tracks, res) in enumerate(ticks):
            paths, n = pl.paths()
            b = pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            got = state(pl)
            assert list(b) == list(best), t
            lens.add((int(n[1][b[1]]), int(n[2][b[2]])))
            check_getter(pl, tracks, "P3 tick %d" % t)
            for p in range(3):
                same(got, res[p], p, "P3 tick %d" % t)
        assert all(a != c for a, c in lens), lens
    finally:
        pl.close()


def test_field_and_repulsive_coupling_together_and_each_removed(pmaf, oracle, scenes, monkeypatch):
    """one handle, six ticks: both couplings, then the repulsive one removed, then the field one removed with the
    repulsive one back, then neither -- the last tick is the uncoupled tick's bits (the oracle knows no tracks)"""
    shape, shift = "M3-cap70-moving", 1
    schedule = ((True, True), (True, True), (True, False), (True, False), (False, True), (False, False))
    scs, (src, scale, anchor), first, ticks = reference_ticks(oracle, scenes, shape, False, shift, repulsive_src=(1, 0),
                                                              schedule=schedule)
    _, _, _, field_only = reference_ticks(oracle, scenes, shape, False, shift)
    assert any(not np.array_equal(ticks[0][2][p]["paths"], field_only[0][2][p]["paths"]) for p in range(2))   # the repulsive track counts
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs, shape)
    try:
        pl.couple_obstacle_tracks(src, scale, anchor, shift)
        pl.couple_tracks([1, 0], shift)
        pl.start()
        now = (True, True)
        for t, (best, tracks, res) in enumerate(ticks):
            pl.stop()
            if schedule[t][0] != now[0]:
                pl.couple_obstacle_tracks(src if schedule[t][0] else None, scale, anchor, shift)
            if schedule[t][1] != now[1]:
                pl.couple_tracks([1, 0] if schedule[t][1] else None, shift)
            now = schedule[t]
            n0 = pl.launch_count()
            b = pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            got = state(pl)
            assert pl.launch_count() == n0 + 1
            assert list(b) == list(best), t
            check_getter(pl, tracks, "schedule tick %d" % t)
            assert [len(r) > 0 for r in pl.get_repulsive_track()] == [now[1]] * 2
            for p in range(2):
                same(got, res[p], p, "schedule tick %d %r" % (t, now))
    finally:
        pl.close()


def test_mixed_handle_keeps_uploaded_tracks_and_offset(pmaf, oracle, scenes, monkeypatch):
    """population 0 coupled, population 1 on uploaded tracks with an offset, in one launch: both rollouts are right. The
    uploads come AFTER the coupling: a short one into population 1's part of the shared buffer, then one longer than
    the capacity (the buffer grows, keeps what it holds and its stride stays straight)."""
    shape = "M3-cap70-moving"
    scs = cref.dual_scenes(scenes, shape, moving=True)
    M = 3
    src, scale, anchor = cref.dual_attach(M)
    src[1, :] = -1
    ora = oracle.OraclePlanner(scs[1], mgr_init_pos=scs[1]["start"])
    ora.set_initial_position(scs[1]["start"])
    ora.rollout()
    p1, n1 = ora.paths()
    ups = fref.tracks_for(scs[1], p1[0], int(n1[0]))
    up, off = ups["Lcap+5"], 1
    assert len(up) == 75
    first, ticks = cref.field_coupled_ticks(oracle, scs, src, scale, anchor, 1, 3, uploaded={1: (up, off)})
    _, plain = cref.field_coupled_ticks(oracle, scs, src, scale, anchor, 1, 1)
    assert not np.array_equal(ticks[0][2][1]["paths"], plain[0][2][1]["paths"])       # the upload counts
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs, shape)
    try:
        pl.couple_obstacle_tracks(src, scale, anchor, 1)
        pl.set_obstacle_tracks([None, ups["short"]])
        pl.set_obstacle_track_offset([0, 2])
        used, uf = pl.get_obstacle_tracks()
        assert len(used[0]) == 0 and list(uf) == [0, 2]
        same_bits(used[1], ups["short"], "short upload")
        pl.set_obstacle_tracks([None, up])
        pl.set_obstacle_track_offset([0, off])
        pl.start()
        got = state(pl)
        used, uf = pl.get_obstacle_tracks()
        assert len(used[0]) == 0 and list(uf) == [0, off]
        same_bits(used[1], up, "uploaded tracks")
        for p in range(2):
            same(got, first[p], p, "mixed first rollout")
        for t, (best, tracks, res) in enumerate(ticks):
            b = pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            got = state(pl)
            assert list(b) == list(best), t
            used, uf = pl.get_obstacle_tracks()
            assert list(uf) == [0, off]
            same_bits(used[0], tracks[0], "mixed tick %d composed" % t)
            same_bits(used[1], up, "mixed tick %d uploaded" % t)
            for p in range(2):
                same(got, res[p], p, "mixed tick %d" % t)
        # the refusals that keep the two sources apart
        _raises(ERR_INVALID, pl.set_obstacle_tracks, [ups["L2"], None])
        _raises(ERR_INVALID, pl.set_obstacle_track_offset, [1, 0])
        both = src.copy()
        both[1, 0] = 0
        _raises(ERR_STATE, pl.couple_obstacle_tracks, both, scale, anchor, 1)
        used, uf = pl.get_obstacle_tracks()
        assert list(uf) == [0, off]
        same_bits(used[0], ticks[-1][1][0], "composed tracks after the refusals")
        same_bits(used[1], up, "uploaded tracks after the refusals")
        # uncoupling leaves the upload; detaching it leaves nothing
        pl.couple_obstacle_tracks(None)
        used, uf = pl.get_obstacle_tracks()
        assert len(used[0]) == 0 and list(uf) == [0, off]
        same_bits(used[1], up, "uploaded tracks after uncoupling")
        pl.set_obstacle_tracks(None)
        assert [len(u) for u in pl.get_obstacle_tracks()[0]] == [0, 0]
    finally:
        pl.close()


def test_adopted_agents_paths_are_followed(pmaf, oracle, scenes, monkeypatch):
    """pmaf_adopt_best between the selection and the reset: the tracks ride on the ADOPTED agents' paths"""
    shape = "M3-cap70-moving"
    scs = sref.dual_scenes(scenes, shape)
    src, scale, anchor = cref.dual_attach(3)
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs, shape)
    try:
        pl.couple_obstacle_tracks(src, scale, anchor, 1)
        pl.rollout()
        for t in range(2):
            paths, n = pl.paths()
            own = pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
            adopt = [(int(own[0]) + 1 + t) % pl.N, (int(own[1]) + 3) % pl.N]
            one_tick(pl, scs, live, "calls", adopt=adopt)
            pl.stop()
            want = expected_tracks(scs, paths, n, adopt, src, scale, anchor, 1)
            check_getter(pl, want, "adopt tick %d" % t)
            wrong = expected_tracks(scs, paths, n, own, src, scale, anchor, 1)
            assert any(not np.array_equal(a, c) for a, c in zip(want, wrong))
    finally:
        pl.close()


def test_tracked_audits_read_the_composed_tracks(pmaf, oracle, scenes, monkeypatch, hip_lib):
    """pmaf_select_clear_tracked(first = [1, 1]) and pmaf_evaluate_paths_tracked on the coupled handle equal
    tracked_audit_reference fed with compose_tracks' output -- the tracks the last launched rollout followed; before the
    first composed launch L = 0: the untracked calls' results"""
    shape = "M3-cap70-moving"
    scs = cref.dual_scenes(scenes, shape, moving=True)
    src, scale, anchor = cref.dual_attach(3)
    live = np.stack([s["obstacles"] for s in scs])
    order = hip_lib.pmaf_eval_order()
    dt, rad = scs[0]["dt"], scs[0]["radius"]
    pl = planner(pmaf, monkeypatch, scs, shape)
    try:
        pl.couple_obstacle_tracks(src, scale, anchor, 1)
        pl.rollout()
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        a, b = pl.select_clear(live, 0.02, 50), pl.select_clear_tracked(live, 0.02, 50)
        for k in a:
            same_bits(b[k], a[k], "before the first composed launch: " + k)
        for t in range(2):
            paths, n = pl.paths()
            best = pl.tick(live, dt, scs[0]["cost_gains"], scs[0]["ws_limits"])
            pl.stop()
        tracks = expected_tracks(scs, paths, n, best, src, scale, anchor, 1)
        check_getter(pl, tracks, "audit")
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        paths, n = pl.paths()
        P, N = pl.P, pl.N
        pl_paths, pl_n, costs = np.asarray(paths).tolist(), np.asarray(n).tolist(), np.asarray(pl.costs()).tolist()
        attached = [t.tolist() for t in tracks]
        for first in ([1, 1], [0, 3]):
            got = pl.evaluate_paths_tracked(live, 0.02, per_obstacle=True, first=first)
            want = tar.audit(pl_paths, pl_n, live.tolist(), attached, first, dt, rad, 0.02, order)
            for k in ("step", "obstacle", "first_violation"):
                np.testing.assert_array_equal(np.asarray(got[k]).reshape(P, N), np.asarray(want[k]), err_msg=k)
            same_bits(np.asarray(got["clearance"]).reshape(P, N), want["clearance"], "audit clearance first %r" % first)
            same_bits(np.asarray(got["per_obstacle"]).reshape(P, N, 4), want["per_obstacle"], "audit per_obstacle first %r" % first)
            for skip in (False, True):
                g = pl.select_clear_tracked(live, 0.02, 50, prev=[1, 1], first=first, skip_trailing=skip)
                w = tar.select_clear(pl_paths, pl_n, live.tolist(), attached, first, costs, dt, rad, 0.02, 50, skip, order, [1, 1])
                for k in ("pick", "rule", "n_clear", "first_violation"):
                    np.testing.assert_array_equal(np.asarray(g[k]).reshape(P), np.asarray(w[k]), err_msg=k)
                for k in ("cost", "clearance"):
                    same_bits(np.asarray(g[k]).reshape(P), w[k], "select %s first %r skip %r" % (k, first, skip))
        untracked = pl.evaluate_paths(live, 0.02)
        assert not np.array_equal(np.asarray(untracked["clearance"]), np.asarray(got["clearance"]))
    finally:
        pl.close()


def test_pair_tick_couples_the_listed_columns(pmaf, oracle, scenes, monkeypatch):
    """shard.DualArmCoupling.pair_tick(field=...): three ticks; each arm's listed columns ride on the path of the OTHER
    arm's member of the adopted pair, composed against the list the tick used; the planner is called once"""
    shape = "M3-cap70-moving"
    scs = sref.dual_scenes(scenes, shape)
    M = 3
    side, link = np.array([0.0, 0.0, 0.25]), np.array([-0.12, 0.0, 0.06])
    field = dict(shift=2, attach=[(0, 1.0, side), (M - 1, 0.8, link)])
    src, scale, anchor = cref.attach(2, M, {(p, c): (1 - p, s, a) for p in range(2) for c, s, a in field["attach"]})
    pl = planner(pmaf, monkeypatch, scs, shape)
    calls = []
    inner = pl.couple_obstacle_tracks
    monkeypatch.setattr(pl, "couple_obstacle_tracks", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])
    try:
        co = pmaf.shard.DualArmCoupling(np.stack([s["obstacles"] for s in scs]))
        pl.rollout()
        for t in range(3):
            pl.stop()
            paths, n = pl.paths()
            out = co.pair_tick(pl, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"], 0.01, adopt=True, field=field)
            pl.stop()
            want = expected_tracks(scs, paths, n, out["pair"], src, scale, anchor, 2, lists=co.obstacles)
            check_getter(pl, want, "pair_tick %d" % t)
            assert (pl.n_points() > 1).all()
        assert len(calls) == 1
        co.pair_tick(pl, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"], 0.01, adopt=True, field=dict(field, shift=3))
        assert len(calls) == 2
        pl.stop()
        inner(None)
    finally:
        pl.close()


# ---- errors and refusals --------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **kw):
    with pytest.raises(Exception) as e:
        fn(*a, **kw)
    assert getattr(e.value, "code", None) == code, e.value
    return str(e.value)


def test_invalid_arguments_and_uncoupling(pmaf, oracle, scenes, monkeypatch, hip_lib):
    import ctypes as C
    scs = cref.dual_scenes(scenes, "M3-cap9")
    M = 3
    src, scale, anchor = cref.dual_attach(M)
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs)
    try:
        def bad(**kw):
            a = dict(src=src.copy(), scale=scale.copy(), anchor=anchor.copy(), shift=1)
            for k, (idx, v) in kw.items():
                if idx is None:
                    a[k] = v
                else:
                    a[k][idx] = v
            return a["src"], a["scale"], a["anchor"], a["shift"]
        _raises(ERR_INVALID, pl.couple_obstacle_tracks, *bad(src=((0, 1), 0)))          # q == p
        _raises(ERR_INVALID, pl.couple_obstacle_tracks, *bad(src=((1, 2), 2)))          # q >= P
        _raises(ERR_INVALID, pl.couple_obstacle_tracks, *bad(src=((1, 1), -2)))         # q < -1
        _raises(ERR_INVALID, pl.couple_obstacle_tracks, *bad(shift=(None, -1)))
        _raises(ERR_INVALID, pl.couple_obstacle_tracks, *bad(scale=((0, 2), np.nan)))
        _raises(ERR_INVALID, pl.couple_obstacle_tracks, *bad(scale=((1, 1), 1e40)))       # (an unattached column's too)
        _raises(ERR_INVALID, pl.couple_obstacle_tracks, *bad(anchor=((1, 0, 2), np.inf)))
        _raises(ERR_INVALID, pl.couple_obstacle_tracks, *bad(anchor=((0, 1, 1), 1e-40)))
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        s32 = np.ascontiguousarray(src, dtype=np.int32)
        for sc_p, an_p in ((None, anchor.ctypes.data_as(dp)), (scale.ctypes.data_as(dp), None)):
            assert hip_lib.pmaf_couple_obstacle_tracks(pl._h, s32.ctypes.data_as(ip), sc_p, an_p, 0) == ERR_INVALID
        assert hip_lib.pmaf_couple_obstacle_tracks(None, None, None, None, 0) == ERR_INVALID
        # nothing was attached by the refused calls
        _raises(ERR_STATE, pl.set_obstacle_track_offset, [0, 0])
        assert [len(t) for t in pl.get_obstacle_tracks()[0]] == [0, 0]
        # coupled: the offset and an upload for a coupled population are refused, all -1 / None uncouple
        pl.couple_obstacle_tracks(src, scale, anchor, 1)
        pl.set_obstacle_track_offset([0, 0])
        _raises(ERR_INVALID, pl.set_obstacle_track_offset, [0, 1])
        _raises(ERR_INVALID, pl.set_obstacle_tracks, np.zeros((2, 4, M, 6)) + 0.5, lengths=[0, 4])
        pl.set_obstacle_tracks(np.zeros((2, 4, M, 6)) + 0.5, lengths=[0, 0])
        pl.couple_obstacle_tracks(np.full((2, M), -1), scale, anchor, 0)
        _raises(ERR_STATE, pl.set_obstacle_track_offset, [0, 0])
        # an uploaded population cannot be coupled
        pl.set_obstacle_tracks(np.zeros((2, 4, M, 6)) + 0.5, lengths=[4, 0])
        _raises(ERR_STATE, pl.couple_obstacle_tracks, src, scale, anchor, 1)
        only1 = src.copy()
        only1[0, :] = -1
        pl.couple_obstacle_tracks(only1, scale, anchor, 1)
        pl.set_obstacle_tracks(None)
        # coupled ticks, then uncoupled: nothing composed is left, and the tick is the two-launch tick again
        # (its bits: the last tick of test_field_and_repulsive_coupling_together_and_each_removed)
        pl.couple_obstacle_tracks(src, scale, anchor, 1)
        pl.start()
        for _ in range(2):
            n0 = pl.launch_count()
            pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            assert pl.launch_count() == n0 + 1
        pl.stop()
        assert [len(t) for t in pl.get_obstacle_tracks()[0]] == [9, 9]
        pl.couple_obstacle_tracks(None)
        assert [len(t) for t in pl.get_obstacle_tracks()[0]] == [0, 0]
        pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
        pl.stop()
        assert [len(t) for t in pl.get_obstacle_tracks()[0]] == [0, 0]
    finally:
        pl.close()


def test_unsupported_routes_refuse_at_attach_and_at_start(pmaf, oracle, scenes, monkeypatch, tmp_path):
    import os
    import subprocess
    # 61 field obstacles: the multi-wave / two-slot kernels
    scs = [scenes.synthetic_scene(cref.N_AGENTS, 8, 61, config_id=11, scene_id=p) for p in range(2)]
    src, scale, anchor = cref.dual_attach(61)
    pl = planner(pmaf, monkeypatch, scs)
    try:
        n0 = pl.launch_count()
        msg = _raises(ERR_STATE, pl.couple_obstacle_tracks, src, scale, anchor, 0)
        assert "obstacle tracks" in msg and ("multi-wave" in msg or "slots" in msg), msg
        assert pl.launch_count() == n0 and [len(t) for t in pl.get_obstacle_tracks()[0]] == [0, 0]
        pl.rollout()       # the handle is as it was: untracked
        assert pl.launch_count() == n0 + 1
    finally:
        pl.close()
    # PMAF_FLAG_CONTRACTED: another arithmetic policy
    scs = cref.dual_scenes(scenes, "M3-cap9")
    src, scale, anchor = cref.dual_attach(3)
    pl = planner(pmaf, monkeypatch, scs, contracted=True)
    try:
        msg = _raises(ERR_STATE, pl.couple_obstacle_tracks, src, scale, anchor, 0)
        assert "obstacle tracks" in msg and "policy" in msg, msg
    finally:
        pl.close()
    # a route that becomes unsupported after the attach: pmaf_start and pmaf_tick refuse, nothing is launched
    code = tmp_path / "ext.hip"
    code.write_text('#include <hip/hip_runtime.h>\nextern "C" __global__ void k_ext_nothing(int) {}\n')
    co = str(tmp_path / "ext.co")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([os.path.join(rocm, "bin", "hipcc"), "--offload-arch=gfx950", "--genco", "-O1", str(code), "-o", co], check=True)
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs)
    try:
        pl.couple_obstacle_tracks(src, scale, anchor, 0)
        pl.external_rollout(co, "k_ext_nothing")
        n0 = pl.launch_count()
        msg = _raises(ERR_STATE, pl.start)
        assert "obstacle tracks" in msg and "external" in msg, msg
        msg = _raises(ERR_STATE, pl.tick, live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
        assert "obstacle tracks" in msg and "external" in msg, msg
        assert pl.launch_count() == n0
        pl.external_rollout(None)
        pl.rollout()
        assert pl.launch_count() == n0 + 1
    finally:
        pl.close()
