"""The obstacle tracks on the GPU (pmaf_set_obstacle_tracks / pmaf_set_obstacle_track_offset / pmaf_get_obstacle_tracks,
k_rollout_w64_ftrack of csrc/pmaf_k_ftrack.hip) through the C-ABI, at tolerance 0 against the composed reference of
tests/field_track_reference.py. The shapes are the repulsive track's (tests/sentinel_track_reference.py); the tracks and
what each reaches are listed in the reference module; tests/test_field_track.py validates the reference on the CPU and
shows that every shape group is sensitive to every rule. The shapes without `moving` have a live list at rest under
tracks that move: the launcher's test for the bodies that assume obstacles at rest reads the live list."""
import os
import subprocess

import numpy as np
import pytest

import field_track_reference as fref
import sentinel_track_reference as sref

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


def planner(pmaf, monkeypatch, scs, shape=None, **kw):
    for k, v in (fref.SHAPES[shape].get("env", {}) if shape else {}).items():
        monkeypatch.setenv(k, v)
    scs = scs if isinstance(scs, list) else [scs]
    pl = pmaf.PmafPlanner(scs if len(scs) > 1 else scs[0], device=0, mgr_init_pos=np.stack([s["start"] for s in scs]), **kw)
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


def reference(oracle, sc, ftracks, first=0, track=None):
    ora = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
    ora.set_initial_position(sc["start"])
    out = fref.compose(ora, oracle.eval_order(), sc, sc["obstacles"], ftracks, first, track)
    ora.evaluate(sc["cost_gains"], sc["ws_limits"])
    out["costs"] = ora.costs()
    return out


def same(got, want, p=0, tag="", latched_only=False, keys=KEYS):
    """latched_only: the handle has rolled out against other tracks before, so the rotation vectors of obstacles THIS
    rollout did not latch are left over from those: compared where the known flag is set"""
    g = {k: np.asarray(got[k][p]) for k in keys}
    w = {k: np.asarray(want[k]) for k in keys}
    if latched_only:
        g["rot"] = g["rot"] * g["known"][..., None]
        w["rot"] = w["rot"] * w["known"][..., None]
    for k in keys:
        print("%s pop %d %s: %d differing entries" % (tag, p, k, int((g[k] != w[k]).sum())))
    for k in keys:
        np.testing.assert_array_equal(g[k], w[k], err_msg="%s pop %d %s" % (tag, p, k))


_UNTRACKED = {}


def case(oracle, scenes, shape):
    """the scene, its untracked oracle rollout and the tracks built from it: computed once per shape, never modified"""
    if shape not in _UNTRACKED:
        sc = fref.build_scene(scenes, shape)
        un = reference(oracle, sc, None)
        _UNTRACKED[shape] = (sc, un, fref.tracks_for(sc, un["paths"][0], int(un["n_points"][0])))
    return _UNTRACKED[shape]


@pytest.mark.parametrize("shape,tname,first", fref.case_list(), ids=lambda v: str(v))
def test_tracked_rollout_equals_the_composed_reference(pmaf, oracle, scenes, monkeypatch, shape, tname, first):
    sc, un, tracks = case(oracle, scenes, shape)
    t = tracks[tname]
    f = fref.resolve_first(first, len(t))
    pl = planner(pmaf, monkeypatch, sc, shape)
    try:
        cfg = pl.launch_config()
        assert cfg["lanes_per_agent"] == 64 and cfg["waves_per_agent"] == 1 and not cfg["priority_slices"]
        pl.set_obstacle_tracks(t)
        if f:
            pl.set_obstacle_track_offset(f)
        n0 = pl.launch_count()
        pl.rollout()
        assert pl.launch_count() == n0 + 1
        got = results(pl, sc)
        used, used_first = pl.get_obstacle_tracks()
        np.testing.assert_array_equal(used[0], t)
        assert list(used_first) == [f]
        same(got, reference(oracle, sc, t, f), tag="%s/%s/%s" % (shape, tname, first))
        assert not np.array_equal(got["paths"][0], un["paths"])
    finally:
        pl.close()


@pytest.mark.parametrize("shape", ["M3-cap70", "M60-cap70", "M59-cap70-moving", "M60-cap70-lds-general-moving"])
def test_straight_line_tracks_and_detach_are_bit_identical_to_untracked(pmaf, oracle, scenes, monkeypatch, shape):
    sc, un, tracks = case(oracle, scenes, shape)
    cap = sc["max_prediction_steps"]
    pl = planner(pmaf, monkeypatch, sc, shape)
    never = planner(pmaf, monkeypatch, sc, shape)
    try:
        pl.rollout()
        plain = results(pl, sc)
        same(plain, un, tag="untracked")
        # the iterated straight lines with the constant velocities as tracks, on the same handle; then from offset 1
        # with the first point doubled
        lines = fref.straight_lines(sc["obstacles"], sc["dt"], cap)
        for given, first in ((lines, 0), (np.concatenate([lines[:1], lines]), 1)):
            pl.set_initial_position(sc["start"])
            pl.set_obstacle_tracks(given)
            pl.set_obstacle_track_offset(first)
            pl.rollout()
            got = results(pl, sc)
            same(got, {k: plain[k][0] for k in KEYS}, tag="straight lines from %d" % first)
            same(got, un, tag="straight lines from %d vs oracle" % first)
        # other tracks, then detached: the next rollout is the one of a handle that never had tracks
        pl.set_initial_position(sc["start"])
        pl.set_obstacle_tracks(tracks["sweep"])
        pl.rollout()
        assert not np.array_equal(results(pl, sc)["paths"], plain["paths"])
        pl.set_obstacle_tracks(None)
        used, first = pl.get_obstacle_tracks()
        assert [len(t) for t in used] == [0] and list(first) == [0]
        for h in (pl, never):
            h.set_initial_position(sc["start"])
            h.rollout()
        a, b = results(pl, sc), results(never, sc)
        same(a, {k: b[k][0] for k in KEYS}, tag="detached", latched_only=True)
        same(a, un, tag="detached vs oracle", latched_only=True)
    finally:
        pl.close()
        never.close()


def test_offset_advances_over_closed_loop_ticks(pmaf, oracle, scenes, monkeypatch):
    """six ticks of the fused pmaf_tick, the offset one further in front of each, against the composer"""
    shape = "M3-cap70"
    sc, un, tracks = case(oracle, scenes, shape)
    t = tracks["sweep"]
    first, ticks = fref.tracked_ticks(oracle, sc, t, 6)
    keys = ("paths", "n_points", "min_obs", "known", "rot", "vel")
    pl = planner(pmaf, monkeypatch, sc, shape)
    try:
        pl.set_obstacle_tracks(t)
        pl.start()
        pl.stop()
        paths, n = pl.paths()
        np.testing.assert_array_equal(n, first["n_points"])
        np.testing.assert_array_equal(paths, first["paths"])
        for k, (best, res) in enumerate(ticks):
            pl.set_obstacle_track_offset(k + 1)
            n0 = pl.launch_count()
            b = pl.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
            pl.stop()
            assert pl.launch_count() == n0 + 1
            assert int(np.asarray(b).reshape(-1)[0]) == int(best), k
            used, used_first = pl.get_obstacle_tracks()
            assert list(used_first) == [k + 1] and len(used[0]) == len(t)
            paths, nn = pl.paths()
            got = dict(paths=paths, n_points=nn, min_obs=pl.min_obs_dist(), known=pl.known(), rot=pl.rot_vecs(), vel=pl.agent_vel())
            same({kk: v[None] for kk, v in got.items()}, res, tag="tick %d" % k, keys=keys)
    finally:
        pl.close()


def test_tracks_per_population_one_untracked(pmaf, oracle, scenes, monkeypatch):
    """P = 2 in one launch: one population tracked, the other at L = 0; then the other way round, with offsets"""
    shape = "M59-cap70"
    scs = [fref.build_scene(scenes, shape, scene_id=p) for p in range(2)]
    uns = [reference(oracle, sc, None) for sc in scs]
    trs = [fref.tracks_for(sc, un["paths"][0], int(un["n_points"][0])) for sc, un in zip(scs, uns)]
    pl = planner(pmaf, monkeypatch, scs)
    try:
        for given, first in (([trs[0]["sweep"], None], [0, 0]), ([None, trs[1]["short"]], [0, 2]),
                             ([trs[0]["L1"], trs[1]["Lcap+5"]], [3, 1])):
            pl.set_initial_position(np.stack([s["start"] for s in scs]))
            pl.set_obstacle_tracks(given)
            pl.set_obstacle_track_offset(first)
            pl.rollout()
            got = results(pl, scs[0])
            used, used_first = pl.get_obstacle_tracks()
            assert list(used_first) == first
            for p in range(2):
                want_t = np.zeros((0, 59, 6)) if given[p] is None else given[p]
                np.testing.assert_array_equal(used[p], want_t)
                same(got, reference(oracle, scs[p], given[p], first[p]), p, tag="per population", latched_only=True)
    finally:
        pl.close()


@pytest.mark.parametrize("shape", ["M3-cap70", "M60-cap70-lds-general-moving"])
def test_field_tracks_together_with_a_repulsive_track(pmaf, oracle, scenes, monkeypatch, shape):
    """both kinds attached (either order), then each detached in turn: the kernel that follows both, the one that follows
    the repulsive track alone, and the field tracks with the trailing obstacle back on its line"""
    sc, un, tracks = case(oracle, scenes, shape)
    rep = sref.tracks_for(sc, un["paths"][0], int(un["n_points"][0]))["in_out"]
    ft = tracks["sweep"]
    pl = planner(pmaf, monkeypatch, sc, shape)
    try:
        pl.set_obstacle_tracks(ft)
        pl.set_repulsive_track(rep)
        pl.set_obstacle_track_offset(1)
        pl.rollout()
        both = results(pl, sc)
        same(both, reference(oracle, sc, ft, 1, rep), tag="both")
        np.testing.assert_array_equal(pl.get_repulsive_track()[0], rep[:sc["max_prediction_steps"]])
        assert not np.array_equal(both["paths"][0], reference(oracle, sc, ft, 1)["paths"])
        pl.set_obstacle_tracks(None)
        pl.set_initial_position(sc["start"])
        pl.rollout()
        same(results(pl, sc), reference(oracle, sc, None, 0, rep), tag="repulsive only", latched_only=True)
        pl.set_obstacle_tracks(ft)
        pl.set_repulsive_track(None)
        pl.set_initial_position(sc["start"])
        pl.rollout()
        same(results(pl, sc), reference(oracle, sc, ft, 0), tag="field only", latched_only=True)
    finally:
        pl.close()


def test_shorter_upload_after_a_longer_one(pmaf, oracle, scenes, monkeypatch):
    """the device buffer only grows: a shorter upload after a longer one reads none of the longer one's points"""
    sc, un, tracks = case(oracle, scenes, "M3-cap70")
    pl = planner(pmaf, monkeypatch, sc)
    try:
        for name in ("Lcap+5", "L2", "short"):
            pl.set_initial_position(sc["start"])
            pl.set_obstacle_tracks(tracks[name])
            pl.rollout()
            got = results(pl, sc)
            used, _ = pl.get_obstacle_tracks()
            np.testing.assert_array_equal(used[0], tracks[name])
            same(got, reference(oracle, sc, tracks[name]), tag=name, latched_only=True)
    finally:
        pl.close()


def _raises(code, fn, *a, **kw):
    with pytest.raises(Exception) as e:
        fn(*a, **kw)
    assert getattr(e.value, "code", None) == code, e.value
    return str(e.value)


def test_invalid_arguments(pmaf, oracle, scenes, monkeypatch):
    scs = [fref.build_scene(scenes, "M3-cap9", scene_id=p) for p in range(2)]
    pl = planner(pmaf, monkeypatch, scs)
    try:
        good = np.zeros((2, 4, 3, 6)) + 0.5
        _raises(ERR_STATE, pl.set_obstacle_track_offset, [0, 0])        # nothing attached yet
        bad = good.copy()
        bad[1, 2, 1, 4] = np.nan
        _raises(ERR_INVALID, pl.set_obstacle_tracks, bad, lengths=[4, 4])
        pl.set_obstacle_tracks(bad, lengths=[4, 2])            # the NaN lies outside len: not read
        _raises(ERR_INVALID, pl.set_obstacle_tracks, good, lengths=[4, -1])
        _raises(ERR_INVALID, pl.set_obstacle_tracks, good, lengths=[5, 1])
        huge = good.copy()
        huge[0, 0, 2, 0] = 1e40
        _raises(ERR_INVALID, pl.set_obstacle_tracks, huge, lengths=[1, 0])
        # a refused call leaves what was attached
        used, first = pl.get_obstacle_tracks()
        assert [len(t) for t in used] == [4, 2]
        _raises(ERR_INVALID, pl.set_obstacle_track_offset, [0, -1])
        pl.set_obstacle_track_offset([2, 7])
        assert list(pl.get_obstacle_tracks()[1]) == [2, 7]
        pl.set_obstacle_tracks(good, lengths=[0, 0])           # all-zero len detaches, the offsets go back to 0
        used, first = pl.get_obstacle_tracks()
        assert [len(t) for t in used] == [0, 0] and list(first) == [0, 0]
        pl.set_obstacle_tracks(None)
    finally:
        pl.close()


def test_unsupported_routes_refuse_at_attach(pmaf, oracle, scenes, monkeypatch):
    # 61 field obstacles: the multi-wave / two-slot kernels
    sc = scenes.synthetic_scene(fref.N_AGENTS, 8, 61, config_id=11)
    pl = planner(pmaf, monkeypatch, sc)
    try:
        n0 = pl.launch_count()
        msg = _raises(ERR_STATE, pl.set_obstacle_tracks, np.zeros((2, 61, 6)) + 0.5)
        assert "obstacle tracks" in msg and ("multi-wave" in msg or "slots" in msg), msg
        assert pl.launch_count() == n0 and [len(t) for t in pl.get_obstacle_tracks()[0]] == [0]
        pl.rollout()       # the handle is as it was: untracked
        assert pl.launch_count() == n0 + 1
    finally:
        pl.close()
    # PMAF_FLAG_CONTRACTED: another arithmetic policy
    sc = fref.build_scene(scenes, "M3-cap9")
    pl = planner(pmaf, monkeypatch, sc, contracted=True)
    try:
        msg = _raises(ERR_STATE, pl.set_obstacle_tracks, np.zeros((2, 3, 6)) + 0.5)
        assert "obstacle tracks" in msg and "policy" in msg, msg
        assert [len(t) for t in pl.get_obstacle_tracks()[0]] == [0]
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
        pl.set_obstacle_tracks(tracks["L2"])
        pl.external_rollout(co, "k_ext_nothing")
        n0 = pl.launch_count()
        msg = _raises(ERR_STATE, pl.start)
        assert "obstacle tracks" in msg and "external" in msg, msg
        assert pl.launch_count() == n0
        pl.external_rollout(None)
        pl.rollout()
        same(results(pl, sc), reference(oracle, sc, tracks["L2"]), tag="after unload")
    finally:
        pl.close()


def test_facade_set_and_advance_obstacle_tracks(pmaf, scenes, tmp_path):
    """tests/cpp/facade_ftracked_tick.cpp calls CfManager::setObstacleTracks once (offset 2), advanceObstacleTracks in
    front of the later planTicks and detaches for the last one; every figure it prints equals the same calls made through
    the binding"""
    import conftest
    N, cap, ticks, L = 12, 101, 5, 40
    sc = scenes.static1_scene(N, cap - 1)
    rvf = tmp_path / "rv.bin"
    np.ascontiguousarray(sc["random_vecs"]).tofile(rvf)
    exe = conftest.exe(os.path.join(conftest.ROOT, "tests", "cpp", "facade_ftracked_tick"))
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    out = subprocess.run([exe, str(N), str(cap), str(ticks), str(rvf), str(L)], capture_output=True, check=True,
                         env=conftest.binary_env(pmaf)).stdout.decode()
    lines = out.strip().split("\n")
    assert len(lines) == ticks
    k = np.arange(L, dtype=np.float64)
    t6 = np.zeros((L, 9, 6))
    t6[:, :, 0:3] = sc["obstacles"][None, :9, 0:3]
    t6[:, :, 0] = sc["obstacles"][None, :9, 0] + 0.0005 * k[:, None]
    t6[:, :, 3:6] = np.stack([np.full(9, 0.05), np.zeros(9), 0.01 * np.arange(9)], axis=1)[None]
    t6[:, 0, 0:3] = np.stack([-0.6 + 0.002 * k, 0.3 - 0.001 * k, np.full(L, 0.75)], axis=1)
    t6[:, 0, 3:6] = [0.2, -0.1, 0.0]
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    plain = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        differs = False
        for h in (pl, plain):
            h.set_initial_position(sc["start"])
            h.start()
        for t in range(ticks):
            if t == 0:
                pl.set_obstacle_tracks(t6)
                pl.set_obstacle_track_offset(2)
            elif t + 1 < ticks:
                pl.set_obstacle_track_offset(2 + t)
            else:
                pl.set_obstacle_tracks(None)
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
        assert differs       # the tracked sphere is in range of this arm: the tracked ticks are not the untracked ones
    finally:
        pl.close()
        plain.close()
