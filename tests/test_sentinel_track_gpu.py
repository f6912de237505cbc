"""The repulsive track on the GPU (pmaf_set_repulsive_track / pmaf_couple_tracks / pmaf_get_repulsive_track,
k_rollout_w64_track and k_track_from_best of csrc/pmaf_k_track.hip) through the C-ABI, at tolerance 0 against the composed
reference of tests/sentinel_track_reference.py. The shapes, the tracks and what each reaches are listed there;
tests/test_sentinel_track.py validates the reference on the CPU and shows that every case is sensitive to the rule."""
import os
import subprocess

import numpy as np
import pytest

import conftest
import pair_clear_reference as pcr
import path_audit_reference as par
import sentinel_track_reference as ref

pytestmark = pytest.mark.gpu

KEYS = ("paths", "n_points", "min_obs", "known", "rot", "vel", "reached", "costs")
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


def test_status_codes():
    import re
    text = open(os.path.join(conftest.ROOT, "include", "pmaf.h")).read()
    assert int(re.search(r"PMAF_ERR_INVALID\s*=\s*(-?\d+)", text).group(1)) == ERR_INVALID
    assert int(re.search(r"PMAF_ERR_STATE\s*=\s*(-?\d+)", text).group(1)) == ERR_STATE


def planner(pmaf, monkeypatch, scs, shape=None):
    for k, v in (ref.SHAPES[shape].get("env", {}) if shape else {}).items():
        monkeypatch.setenv(k, v)
    scs = scs if isinstance(scs, list) else [scs]
    pl = pmaf.PmafPlanner(scs if len(scs) > 1 else scs[0], device=0, mgr_init_pos=np.stack([s["start"] for s in scs]))
    pl.set_initial_position(np.stack([s["start"] for s in scs]))
    return pl


def results(pl, sc):
    """the rollout's results of a handle, [P][...] (population axis kept)"""
    pl.stop()
    paths, n = pl.paths()
    out = dict(paths=paths, n_points=n, min_obs=pl.min_obs_dist(), known=pl.known(), rot=pl.rot_vecs(), vel=pl.agent_vel(),
               reached=pl.success())
    pl.evaluate(sc["cost_gains"], sc["ws_limits"])
    out["costs"] = pl.costs()
    if pl.P == 1:
        out = {k: v[None] for k, v in out.items()}
    return out


def reference(oracle, sc, track):
    ora = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
    ora.set_initial_position(sc["start"])
    out = ref.compose(ora, oracle.eval_order(), sc, sc["obstacles"], track)
    ora.evaluate(sc["cost_gains"], sc["ws_limits"])
    out["costs"] = ora.costs()
    return out


def same(got, want, p=0, tag="", latched_only=False):
    """latched_only: the handle has rolled out against other tracks before, so the rotation vectors of obstacles THIS
    rollout did not latch are left over from those (the reference's agents keep theirs the same way): compared where the
    known flag is set"""
    g = {k: np.asarray(got[k][p]) for k in KEYS}
    w = {k: np.asarray(want[k]) for k in KEYS}
    if latched_only:
        g["rot"] = g["rot"] * g["known"][..., None]
        w["rot"] = w["rot"] * w["known"][..., None]
    for k in KEYS:
        print("%s pop %d %s: %d differing entries" % (tag, p, k, int((g[k] != w[k]).sum())))
    for k in KEYS:
        np.testing.assert_array_equal(g[k], w[k], err_msg="%s pop %d %s" % (tag, p, k))


_UNTRACKED = {}


def case(oracle, scenes, shape):
    """the scene, its untracked oracle rollout and the tracks built from it: computed once per shape, never modified"""
    if shape not in _UNTRACKED:
        sc = ref.build_scene(scenes, shape)
        un = reference(oracle, sc, None)
        _UNTRACKED[shape] = (sc, un, ref.tracks_for(sc, un["paths"][0], int(un["n_points"][0])))
    return _UNTRACKED[shape]


def used_track(track, cap):
    return np.asarray(track)[:min(len(track), cap)]


@pytest.mark.parametrize("shape,tname", ref.case_list(), ids=lambda v: v)
def test_tracked_rollout_equals_the_composed_reference(pmaf, oracle, scenes, monkeypatch, shape, tname):
    sc, un, tracks = case(oracle, scenes, shape)
    pl = planner(pmaf, monkeypatch, sc, shape)
    try:
        cfg = pl.launch_config()
        assert cfg["lanes_per_agent"] == 64 and cfg["waves_per_agent"] == 1 and not cfg["priority_slices"]
        pl.set_repulsive_track(tracks[tname])
        n0 = pl.launch_count()
        pl.rollout()
        assert pl.launch_count() == n0 + 1
        got = results(pl, sc)
        np.testing.assert_array_equal(pl.get_repulsive_track()[0], used_track(tracks[tname], sc["max_prediction_steps"]))
        same(got, reference(oracle, sc, tracks[tname]), tag="%s/%s" % (shape, tname))
        if tname == "far":     # through the loop without code for the obstacle: the untracked rollout with a far sphere
            sc2 = dict(sc, obstacles=sc["obstacles"].copy())
            sc2["obstacles"][-1, 0:6] = [100.0, 100.0, 100.0, 0.0, 0.0, 0.0]
            same(got, reference(oracle, sc2, None), tag="far sphere")
        else:
            assert not np.array_equal(got["paths"][0], un["paths"])
    finally:
        pl.close()


@pytest.mark.parametrize("shape", ["M3-cap70", "M60-cap70", "M59-cap70-moving", "M60-cap70-lds-general-moving"])
def test_straight_line_track_and_detach_are_bit_identical_to_untracked(pmaf, oracle, scenes, monkeypatch, shape):
    sc, un, tracks = case(oracle, scenes, shape)
    pl = planner(pmaf, monkeypatch, sc, shape)
    never = planner(pmaf, monkeypatch, sc, shape)
    try:
        pl.rollout()
        plain = results(pl, sc)
        same(plain, un, tag="untracked")
        # the iterated straight line as a track, on the same handle
        pl.set_initial_position(sc["start"])
        pl.set_repulsive_track(ref.straight_line(sc["obstacles"], sc["dt"], sc["max_prediction_steps"]))
        pl.rollout()
        same(results(pl, sc), {k: plain[k][0] for k in KEYS}, tag="straight line")
        # another track, then detached: the next rollout is the one of a handle that never had a track
        pl.set_initial_position(sc["start"])
        pl.set_repulsive_track(tracks["in_out"])
        pl.rollout()
        assert not np.array_equal(results(pl, sc)["paths"], plain["paths"])
        pl.set_repulsive_track(None)
        assert [len(t) for t in pl.get_repulsive_track()] == [0]
        for h in (pl, never):
            h.set_initial_position(sc["start"])
            h.rollout()
        a, b = results(pl, sc), results(never, sc)
        same(a, {k: b[k][0] for k in KEYS}, tag="detached", latched_only=True)
        same(a, un, tag="detached vs oracle", latched_only=True)
    finally:
        pl.close()
        never.close()


def test_tracks_per_population_one_untracked(pmaf, oracle, scenes, monkeypatch):
    shape = "M59-cap70"
    scs = [ref.build_scene(scenes, shape, scene_id=p) for p in range(2)]
    uns = [reference(oracle, sc, None) for sc in scs]
    trs = [ref.tracks_for(sc, un["paths"][0], int(un["n_points"][0])) for sc, un in zip(scs, uns)]
    pl = planner(pmaf, monkeypatch, scs)
    try:
        for given in ([trs[0]["in_out"], None], [None, trs[1]["short"]], [trs[0]["L1"], trs[1]["Lcap+5"]]):
            pl.set_initial_position(np.stack([s["start"] for s in scs]))
            pl.set_repulsive_track(given)
            pl.rollout()
            got = results(pl, scs[0])
            used = pl.get_repulsive_track()
            for p in range(2):
                want_t = np.zeros((0, 3)) if given[p] is None else used_track(given[p], scs[p]["max_prediction_steps"])
                np.testing.assert_array_equal(used[p], want_t)
                same(got, reference(oracle, scs[p], given[p]), p, tag="per population", latched_only=True)
    finally:
        pl.close()


@pytest.mark.parametrize("style", ["tick", "calls"])
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_coupled_ticks(pmaf, oracle, scenes, monkeypatch, shift, style):
    """six ticks of two populations coupled mutually -- the fused pmaf_tick, or the node's five calls, whose reset cuts the
    paths before the rollout is launched -- against the composer, which reads the oracle's selected path each tick; the
    first rollout, before any selection, runs untracked"""
    scs = ref.dual_scenes(scenes)
    first, ticks = ref.coupled_ticks(oracle, scs, [1, 0], shift, 6)
    _, plain = ref.coupled_ticks(oracle, scs, None, 0, 1)
    assert not np.array_equal(ticks[0][2][0]["paths"], plain[0][2][0]["paths"])      # the coupling matters from the first tick on
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs)
    try:
        pl.couple_tracks([1, 0], shift)
        pl.start()
        pl.stop()
        assert [len(t) for t in pl.get_repulsive_track()] == [0, 0]
        paths, n = pl.paths()
        for p in range(2):
            np.testing.assert_array_equal(n[p], first[p]["n_points"])
            np.testing.assert_array_equal(paths[p], first[p]["paths"])
        for t, (best, tracks, res) in enumerate(ticks):
            n0 = pl.launch_count()
            if style == "tick":
                b = pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            else:
                pl.stop()
                b = pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
                pl.move_real(live, scs[0]["dt"], 1, b)
                pos, vel, _ = pl.real_state()
                pl.reset_agents(pos, vel, live)
                pl.start()
            pl.stop()
            assert pl.launch_count() == n0 + 1
            assert list(b) == list(best), t
            used = pl.get_repulsive_track()
            paths, n = pl.paths()
            got = dict(paths=paths, n_points=n, min_obs=pl.min_obs_dist(), known=pl.known(), rot=pl.rot_vecs(), vel=pl.agent_vel())
            for p in range(2):
                np.testing.assert_array_equal(used[p], tracks[p], err_msg="tick %d pop %d track" % (t, p))
                for k in got:
                    print("tick %d pop %d %s: %d differing entries" % (t, p, k, int((got[k][p] != res[p][k]).sum())))
                for k in got:
                    np.testing.assert_array_equal(got[k][p], res[p][k], err_msg="tick %d pop %d %s" % (t, p, k))
        # uncoupled again: the two-launch tick of a handle without tracks
        pl.couple_tracks(None)
        assert [len(t) for t in pl.get_repulsive_track()] == [0, 0]
    finally:
        pl.close()


def test_upload_between_reset_and_start_keeps_the_taken_tracks(pmaf, oracle, scenes, monkeypatch):
    """Regression, the shortest form of what tests/test_sequence_gpu.py's seeded sequences found (the model's mutant
    upload_drops_taken is the library as it was): population 1 follows population 0's
    selected path; in the five-call tick pmaf_set_repulsive_track (an upload for population 0) comes between
    pmaf_reset_agents, which took the selected path, and pmaf_start. The upload used to rebuild the whole device buffer
    -- population 1's length became 0 while the handle still counted the track as taken, so the launch took nothing
    and population 1 rolled out untracked. The taken track stays: the getter shows it before and after the launch, and
    population 1's rollout is bit for bit that of a twin handle that made no upload."""
    scs = ref.dual_scenes(scenes)
    sc = scs[0]
    live = np.stack([s["obstacles"] for s in scs])
    up = ref.tracks_for(sc, *_first_path(oracle, sc))["L2"]
    twins = [planner(pmaf, monkeypatch, scs) for _ in range(2)]
    try:
        got = []
        for k, pl in enumerate(twins):
            pl.couple_tracks([-1, 0], 1)
            pl.start()
            pl.tick(live, sc["dt"], sc["cost_gains"], sc["ws_limits"])
            pl.stop()
            paths, n = pl.paths()
            b = pl.evaluate(sc["cost_gains"], sc["ws_limits"])
            pl.move_real(live, sc["dt"], 1, b)
            pos, vel, _ = pl.real_state()
            pl.reset_agents(pos, vel, live)
            taken = ref.coupled_track(paths[0][int(b[0])], int(n[0][int(b[0])]), True, 1)
            assert len(taken) > 3
            if k == 0:
                pl.set_repulsive_track([up, None])
            for when in ("before", "after"):
                used = pl.get_repulsive_track()
                np.testing.assert_array_equal(used[1], taken, err_msg="handle %d, %s the launch: the taken track" % (k, when))
                np.testing.assert_array_equal(used[0], up if k == 0 else np.zeros((0, 3)), err_msg="handle %d, %s the launch: the upload" % (k, when))
                pl.start()
                pl.stop()
            paths, n = pl.paths()
            got.append((paths, n))
        np.testing.assert_array_equal(got[0][1][1], got[1][1][1])
        np.testing.assert_array_equal(got[0][0][1], got[1][0][1])
        assert not np.array_equal(got[0][0][0], got[1][0][0])       # (population 0 did follow its upload)
    finally:
        for pl in twins:
            pl.close()


def _first_path(oracle, sc):
    un = reference(oracle, sc, None)
    return un["paths"][0], int(un["n_points"][0])


def _raises(code, fn, *a, **kw):
    with pytest.raises(Exception) as e:
        fn(*a, **kw)
    assert getattr(e.value, "code", None) == code, e.value
    return str(e.value)


def test_unsupported_routes_refuse_at_attach(pmaf, oracle, scenes, monkeypatch):
    track = np.array([[0.0, 0.3, 0.7], [0.0, 0.31, 0.7]])
    # 61 field obstacles: the multi-wave / two-slot kernels
    sc = scenes.synthetic_scene(ref.N_AGENTS, 8, 61, config_id=11)
    pl = planner(pmaf, monkeypatch, sc)
    try:
        n0 = pl.launch_count()
        msg = _raises(ERR_STATE, pl.set_repulsive_track, track)
        assert "multi-wave" in msg or "slots" in msg, msg
        assert pl.launch_count() == n0 and [len(t) for t in pl.get_repulsive_track()] == [0]
        pl.rollout()       # the handle is as it was: untracked
        assert pl.launch_count() == n0 + 1
    finally:
        pl.close()
    scs = [scenes.synthetic_scene(ref.N_AGENTS, 8, 61, config_id=11, scene_id=p) for p in range(2)]
    pl = planner(pmaf, monkeypatch, scs)
    try:
        _raises(ERR_STATE, pl.couple_tracks, [1, 0], 0)
    finally:
        pl.close()
    # the generic kernel, forced
    monkeypatch.setenv("PMAF_FORCE_GENERIC", "1")
    pl = planner(pmaf, monkeypatch, ref.build_scene(scenes, "M3-cap9"))
    try:
        n0 = pl.launch_count()
        assert "generic" in _raises(ERR_STATE, pl.set_repulsive_track, track)
        assert pl.launch_count() == n0
    finally:
        pl.close()
    monkeypatch.delenv("PMAF_FORCE_GENERIC")
    # another arithmetic policy
    sc = ref.build_scene(scenes, "M3-cap9")
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"], ieee_sequences=True)
    try:
        assert "policy" in _raises(ERR_STATE, pl.set_repulsive_track, track)
    finally:
        pl.close()


def test_invalid_arguments(pmaf, oracle, scenes, monkeypatch):
    scs = [ref.build_scene(scenes, "M3-cap9", scene_id=p) for p in range(2)]
    pl = planner(pmaf, monkeypatch, scs)
    try:
        good = np.zeros((2, 4, 3)) + 0.5
        bad = good.copy()
        bad[1, 2, 1] = np.nan
        _raises(ERR_INVALID, pl.set_repulsive_track, bad, lengths=[4, 4])
        pl.set_repulsive_track(bad, lengths=[4, 2])            # the NaN lies outside len: not read
        _raises(ERR_INVALID, pl.set_repulsive_track, good, lengths=[4, -1])
        _raises(ERR_INVALID, pl.set_repulsive_track, good, lengths=[5, 1])
        huge = good.copy()
        huge[0, 0, 0] = 1e40
        _raises(ERR_INVALID, pl.set_repulsive_track, huge, lengths=[1, 0])
        _raises(ERR_INVALID, pl.couple_tracks, [0, 0], 0)       # src_pop == p
        _raises(ERR_INVALID, pl.couple_tracks, [1, 2], 0)       # q >= P
        _raises(ERR_INVALID, pl.couple_tracks, [1, 0], -1)
        pl.couple_tracks([1, -1], 2)
        pl.couple_tracks(None)
        pl.set_repulsive_track(None)
        assert [len(t) for t in pl.get_repulsive_track()] == [0, 0]
    finally:
        pl.close()


def test_route_that_becomes_unsupported_fails_at_start(pmaf, oracle, scenes, monkeypatch, tmp_path):
    """an external rollout kernel loaded after the attach: pmaf_start refuses, nothing is launched; unloading it restores
    the tracked rollout"""
    src = tmp_path / "ext.hip"
    src.write_text('#include <hip/hip_runtime.h>\nextern "C" __global__ void k_ext_nothing(int) {}\n')
    co = str(tmp_path / "ext.co")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([os.path.join(rocm, "bin", "hipcc"), "--offload-arch=gfx950", "--genco", "-O1", str(src), "-o", co], check=True)
    sc, un, tracks = case(oracle, scenes, "M3-cap9")
    pl = planner(pmaf, monkeypatch, sc)
    try:
        pl.set_repulsive_track(tracks["L2"])
        pl.external_rollout(co, "k_ext_nothing")
        n0 = pl.launch_count()
        assert "external" in _raises(ERR_STATE, pl.start)
        assert pl.launch_count() == n0
        pl.external_rollout(None)
        pl.rollout()
        same(results(pl, sc), reference(oracle, sc, tracks["L2"]), tag="after unload")
    finally:
        pl.close()


def test_audits_run_unchanged_on_tracked_paths(pmaf, oracle, scenes, monkeypatch):
    scs = ref.dual_scenes(scenes)
    order = oracle.eval_order()
    live = np.stack([s["obstacles"] for s in scs])
    pl = planner(pmaf, monkeypatch, scs)
    try:
        pl.couple_tracks([1, 0], 1)
        pl.rollout()
        for _ in range(2):
            pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
        pl.stop()
        assert [len(t) for t in pl.get_repulsive_track()] == [scs[0]["max_prediction_steps"] - 1] * 2
        paths, n = pl.paths()
        got = pl.evaluate_paths(live, 0.05)
        want = par.audit(paths.tolist(), n.tolist(), live.tolist(), scs[0]["dt"], scs[0]["radius"], 0.05, order)
        for k in ("clearance", "step", "obstacle", "first_violation"):
            np.testing.assert_array_equal(got[k], np.asarray(want[k]), err_msg=k)
        pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        costs = pl.costs()
        horizon = scs[0]["max_prediction_steps"]
        g = pl.select_pair_clear(0, 1, live, 0.02, horizon, 0.15, 0.01, skip_trailing=1)
        w = pcr.select_pair_clear(paths.tolist(), n.tolist(), live.tolist(), costs.tolist(), scs[0]["dt"], scs[0]["radius"], 0, 1,
                                  0.02, horizon, 1, 0.15, 0.01, None, None, order)
        assert tuple(g["pair"]) == tuple(w["pair"]) and g["rule"] == w["rule"] and g["n_feasible"] == w["n_feasible"]
        assert g["clearance"] == w["clearance"] and g["cost"] == w["cost"]
    finally:
        pl.close()


def test_pair_tick_couples_the_arms(pmaf, oracle, scenes, monkeypatch):
    """shard.DualArmCoupling.pair_tick(tracks=shift): each arm's rollout follows the path of the OTHER arm's member of the
    adopted pair, from point `shift` on; the sphere at the last set-point stays in the live list"""
    scs = ref.dual_scenes(scenes)
    pl = planner(pmaf, monkeypatch, scs)
    try:
        co = pmaf.shard.DualArmCoupling(np.stack([s["obstacles"] for s in scs]))
        pl.rollout()
        for t in range(3):
            pl.stop()
            paths, n = pl.paths()
            before = np.array(pl.real_state()[0], copy=True)
            out = co.pair_tick(pl, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"], 0.01, adopt=True, tracks=2)
            pl.stop()
            i, j = out["pair"]
            used = pl.get_repulsive_track()
            np.testing.assert_array_equal(used[0], paths[1, j, 2:n[1, j]])
            np.testing.assert_array_equal(used[1], paths[0, i, 2:n[0, i]])
            np.testing.assert_array_equal(co.obstacles[:, -1, 0:3], before[::-1])
            assert (co.obstacles[:, -1, 6] == 0.1).all() and (pl.n_points() > 1).all()
        pl.couple_tracks(None)
    finally:
        pl.close()


def test_facade_set_repulsive_track(pmaf, scenes, tmp_path):
    """tests/cpp/facade_tracked_tick.cpp calls CfManager::setRepulsiveTrack in front of planTick over 5 ticks (the last one
    detached); every figure it prints equals the same calls made through the binding"""
    N, cap, ticks, L = 12, 101, 5, 40
    sc = scenes.static1_scene(N, cap - 1)
    rvf = tmp_path / "rv.bin"
    np.ascontiguousarray(sc["random_vecs"]).tofile(rvf)
    exe = conftest.exe(os.path.join(conftest.ROOT, "tests", "cpp", "facade_tracked_tick"))
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    out = subprocess.run([exe, str(N), str(cap), str(ticks), str(rvf), str(L)], capture_output=True, check=True,
                         env=conftest.binary_env(pmaf)).stdout.decode()
    lines = out.strip().split("\n")
    assert len(lines) == ticks
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    plain = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        differs = False
        for h in (pl, plain):
            h.set_initial_position(sc["start"])
            h.start()
        for t in range(ticks):
            k = np.arange(t, t + L, dtype=np.float64)
            pl.set_repulsive_track(np.stack([-0.6 + 0.002 * k, 0.3 - 0.001 * k, np.full(L, 0.75)], axis=1) if t + 1 < ticks else None)
            row = []
            for h in (pl, plain):
                b = h.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
                h.stop()
                paths, n = h.paths()
                row.append((b, int(n[b]), h.last_next_pos[0].copy(), paths[b, n[b] - 1].copy()))
            f = lines[t].split()
            b, nb, nxt, end = row[0]
            assert [int(v) for v in f[:3]] == [t, b, nb]
            np.testing.assert_array_equal(np.array(f[3:6], dtype=float), nxt)
            np.testing.assert_array_equal(np.array(f[6:9], dtype=float), end)
            differs = differs or not np.array_equal(end, row[1][3])
        assert differs       # the track is in range of this arm: the tracked ticks are not the untracked ones
    finally:
        pl.close()
        plain.close()
