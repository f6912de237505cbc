"""The obstacle tracks' device-memory source on the GPU (pmaf_set_obstacle_tracks_device, k_ftingest_check /
k_ftingest_store of csrc/pmaf_k_ftingest.hip) through the binding, at tolerance 0 against tests/track_ingest_reference.py:
the ingested points are the reference's bit for bit, and every rollout equals the one of a twin handle that was handed
the reference's points through the HOST call. Device buffers come from torch. No test hands the library a pointer or an
extent the device cannot read. tests/test_track_ingest.py shows on the CPU that the cases tell the rule from its mutants
and that the inputs pass the validation."""
import os
import re
import subprocess

import numpy as np
import pytest

import field_couple_reference as cref
import sentinel_track_reference as sref
import track_ingest_reference as tref

pytestmark = pytest.mark.gpu

KEYS = ("paths", "n_points", "min_obs", "known", "rot", "vel", "reached", "costs")
ERR_INVALID, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("PMAF_SUM", "PMAF_FORCE_GENERIC", "PMAF_PLAIN_STEP", "PMAF_MW", "PMAF_W64_SLICE"):
        monkeypatch.delenv(k, raising=False)


def scene_for(scenes, shape, scene_id=0):
    if shape in sref.SHAPES:
        sc = sref.build_scene(scenes, shape, scene_id)
    else:
        M, cap = tref.PARITY_SHAPES[shape]
        sc = scenes.synthetic_scene(sref.N_AGENTS, cap - 1, M, config_id=11, scene_id=scene_id, dynamic=False)
    assert sc["dt"] == tref.DT
    if shape in tref.PARITY_SHAPES:
        assert (len(sc["obstacles"]) - 1, sc["max_prediction_steps"]) == tref.PARITY_SHAPES[shape]
    return sc


def planner(pmaf, scs, **kw):
    scs = scs if isinstance(scs, list) else [scs]
    pl = pmaf.PmafPlanner(scs if len(scs) > 1 else scs[0], device=0, mgr_init_pos=np.stack([s["start"] for s in scs]), **kw)
    pl.set_initial_position(np.stack([s["start"] for s in scs]))
    pl.scs = scs
    return pl


def roll(pl):
    """a rollout from the start state and its results, [P][...]"""
    sc = pl.scs[0]
    pl.set_initial_position(np.stack([s["start"] for s in pl.scs]))
    pl.rollout()
    paths, n = pl.paths()
    out = dict(paths=paths, n_points=n, min_obs=pl.min_obs_dist(), known=pl.known(), rot=pl.rot_vecs(), vel=pl.agent_vel(),
               reached=pl.success())
    pl.evaluate(sc["cost_gains"], sc["ws_limits"])
    out["costs"] = pl.costs()
    if pl.P == 1:
        out = {k: np.asarray(v)[None] for k, v in out.items()}
    # rotation vectors of obstacles this rollout did not latch are left over from earlier ones
    out["rot"] = np.asarray(out["rot"]) * np.asarray(out["known"])[..., None]
    return out


def same(a, b, tag=""):
    for k in KEYS:
        print("%s %s: %d differing entries" % (tag, k, int((np.asarray(a[k]) != np.asarray(b[k])).sum())))
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg="%s %s" % (tag, k))


def bits(a, b, tag=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    n = int((a.view(np.uint64) != b.view(np.uint64)).sum())
    print("%s: %d entries differ in bits" % (tag, n))
    assert n == 0, tag


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _raises(code, fn, *a, **kw):
    with pytest.raises(Exception) as e:
        fn(*a, **kw)
    assert getattr(e.value, "code", None) == code, e.value
    return str(e.value)


@pytest.mark.parametrize("shape", list(tref.PARITY_SHAPES))
@pytest.mark.parametrize("dtype,c", tref.PAIRS, ids=lambda v: str(v))
def test_ingested_points_and_rollout_equal_the_host_twin(pmaf, scenes, torch, shape, dtype, c):
    sc = scene_for(scenes, shape)
    src = tref.parity_source(shape, dtype, c)
    if (dtype, c) == ("f64", 6):
        src[0, 0, 0], src[1, -1, 4], src[2, 0, 5] = -0.0, 2.0 ** -100, -2.0 ** 100
    want = tref.expected_tracks(src, c, sc["dt"])
    pl, twin = planner(pmaf, sc), planner(pmaf, sc)
    try:
        t = dev(torch, src)
        n0 = pl.launch_count()
        pl.set_obstacle_tracks_device(t)
        assert pl.launch_count() == n0
        used, first = pl.get_obstacle_tracks()
        bits(used[0], want, "getter")
        assert list(first) == [0]
        twin.set_obstacle_tracks(src.astype(np.float64) if c == 6 else want)
        bits(twin.get_obstacle_tracks()[0][0], want, "twin getter")
        same(roll(pl), roll(twin), "%s %s/%d" % (shape, dtype, c))
    finally:
        pl.close()
        twin.close()


def test_tracked_rollout_is_not_the_untracked_one(pmaf, scenes, torch):
    """the parity sources are in range of the agents: following them changes the paths"""
    sc = scene_for(scenes, "M59-cap70-moving")
    pl = planner(pmaf, sc)
    try:
        un = roll(pl)
        pl.set_obstacle_tracks_device(dev(torch, tref.parity_source("M59-cap70-moving", "f32", 3)))
        assert not np.array_equal(roll(pl)["paths"], un["paths"])
    finally:
        pl.close()


def test_lengths_offset_and_padding(pmaf, scenes, torch):
    sc = scene_for(scenes, "M3-cap9")
    cap, M = sc["max_prediction_steps"], 3
    pl, twin = planner(pmaf, sc), planner(pmaf, sc)
    try:
        for dtype, c in tref.PAIRS:
            for L, first in ((1, 0), (2, 0), (2, 1), (cap, 0), (cap + 5, 3)):
                src = tref.make_source(M, L, c, dtype, seed=5)
                want = tref.expected_tracks(src, c, sc["dt"])
                if c == 3:
                    assert not want[-1, :, 3:6].any() and not np.signbit(want[-1, :, 3:6]).any()
                pl.set_obstacle_tracks_device(dev(torch, src))
                twin.set_obstacle_tracks(want)
                for h in (pl, twin):
                    assert list(h.get_obstacle_tracks()[1]) == [0]      # every offset becomes 0
                    h.set_obstacle_track_offset(first)
                bits(pl.get_obstacle_tracks()[0][0], want, "L=%d" % L)
                same(roll(pl), roll(twin), "%s/%d L=%d first=%d" % (dtype, c, L, first))
                # max_len > len with NaN and a huge value in the padding: accepted, results unchanged
                pad = np.full((1, L + 3, M, c), np.nan, dtype=src.dtype)
                pad[0, L:, 0] = 1e300 if dtype == "f64" else 1e38
                pad[0, :L] = src
                pl.set_obstacle_tracks_device(dev(torch, pad), [L])
                pl.set_obstacle_track_offset(first)
                bits(pl.get_obstacle_tracks()[0][0], want, "padded L=%d" % L)
                same(roll(pl), roll(twin), "padded")
    finally:
        pl.close()
        twin.close()


def test_per_population_lengths_one_untracked(pmaf, scenes, torch):
    shape = "M59-cap70-moving"
    scs = [scene_for(scenes, shape, scene_id=p) for p in range(2)]
    L, M = 20, 59
    pl, twin, never = planner(pmaf, scs), planner(pmaf, scs), planner(pmaf, scs)
    try:
        un = roll(never)
        src = np.stack([tref.make_source(M, L, 3, "f32", seed=8 + p) for p in range(2)])
        for lens in ((L, 0), (0, L), (L, L - 7)):
            pl.set_obstacle_tracks_device(dev(torch, src), lens)
            want = [tref.expected_tracks(src[p, :lens[p]], 3, scs[0]["dt"]) for p in range(2)]
            twin.set_obstacle_tracks(want)
            used, _ = pl.get_obstacle_tracks()
            for p in range(2):
                bits(used[p], want[p], "pop %d" % p)
            got = roll(pl)
            same(got, roll(twin), str(lens))
            for p in range(2):
                if lens[p] == 0:
                    for k in KEYS:
                        np.testing.assert_array_equal(got[k][p], un[k][p], err_msg="untracked pop %d %s" % (p, k))
                else:
                    assert not np.array_equal(got["paths"][p], un["paths"][p])
    finally:
        for h in (pl, twin, never):
            h.close()


def test_sources_that_are_not_16_byte_aligned(pmaf, scenes, torch):
    sc = scene_for(scenes, "M3-cap9")
    pl = planner(pmaf, sc)
    try:
        for dtype, c in tref.PAIRS:
            src = tref.make_source(3, 7, c, dtype, seed=11)
            buf = torch.zeros(src.size + 1, dtype=dev(torch, src).dtype, device="cuda:0")
            assert buf.data_ptr() % 16 == 0
            view = buf[1:]
            view.copy_(dev(torch, src).reshape(-1))
            t = view.reshape(src.shape)
            assert t.data_ptr() % 16 == src.itemsize and t.is_contiguous()
            pl.set_obstacle_tracks_device(t)
            bits(pl.get_obstacle_tracks()[0][0], tref.expected_tracks(src, c, sc["dt"]), "%s/%d" % (dtype, c))
    finally:
        pl.close()


def test_buffer_life_shorter_after_longer_and_host_device_alternation(pmaf, scenes, torch):
    sc = scene_for(scenes, "M3-cap9")
    pl, twin = planner(pmaf, sc), planner(pmaf, sc)
    try:
        for how, L, c in (("dev", 14, 3), ("dev", 2, 6), ("host", 9, 6), ("dev", 5, 3), ("host", 3, 6), ("dev", 14, 6)):
            src = tref.make_source(3, L, c, "f64", seed=20 + L)
            want = tref.expected_tracks(src, c, sc["dt"])
            if how == "dev":
                pl.set_obstacle_tracks_device(dev(torch, src))
            else:
                pl.set_obstacle_tracks(want)
            twin.set_obstacle_tracks(want)
            bits(pl.get_obstacle_tracks()[0][0], want, "%s L=%d" % (how, L))
            same(roll(pl), roll(twin), "%s L=%d" % (how, L))
        # every len == 0 detaches, as in the host call
        pl.set_obstacle_tracks_device(dev(torch, src), [0])
        twin.set_obstacle_tracks(None)
        assert [len(t) for t in pl.get_obstacle_tracks()[0]] == [0]
        same(roll(pl), roll(twin), "detached")
    finally:
        pl.close()
        twin.close()


def test_coupled_handle_grows_and_keeps_the_composed_points(pmaf, scenes, torch):
    """population 0 rides on population 1's selected path; population 1 is uploaded from the device with a max_len that
    makes the shared buffer grow. The same sequence through the host call on a twin."""
    scs = cref.dual_scenes(scenes, "M3-cap70")
    M, cap = 3, scs[0]["max_prediction_steps"]
    src_pop, scale, anchor = cref.attach(2, M, {(0, 0): (1, 1.0, cref.SIDE)})
    live = np.stack([s["obstacles"] for s in scs])
    pl, twin = planner(pmaf, scs), planner(pmaf, scs)
    up = tref.make_source(M, cap + 10, 3, "f32", seed=31)
    pad = np.zeros((2, cap + 10, M, 3), dtype=np.float32)
    pad[1] = up
    want = tref.expected_tracks(up, 3, scs[0]["dt"])
    try:
        for h in (pl, twin):
            h.couple_obstacle_tracks(src_pop, scale, anchor, 1)
            h.start()
            for _ in range(2):
                h.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            h.stop()
        before, _ = pl.get_obstacle_tracks()
        assert len(before[0]) == cap and len(before[1]) == 0
        _raises(ERR_INVALID, pl.set_obstacle_tracks_device, dev(torch, pad), [3, cap + 10])     # a coupled population with len > 0
        pl.set_obstacle_tracks_device(dev(torch, pad), [0, cap + 10])
        twin.set_obstacle_tracks([None, want])
        for h in (pl, twin):
            used, first = h.get_obstacle_tracks()
            bits(used[0], before[0], "composed points survive the grow")
            bits(used[1], want, "uploaded")
            assert list(first) == [0, 0]
        for _ in range(2):
            a = pl.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            b = twin.tick(live, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
            np.testing.assert_array_equal(a, b)
        for h in (pl, twin):
            h.stop()
        pa, na = pl.paths()
        pb, nb = twin.paths()
        np.testing.assert_array_equal(na, nb)
        np.testing.assert_array_equal(pa, pb)
        ua, ub = pl.get_obstacle_tracks()[0], twin.get_obstacle_tracks()[0]
        for p in range(2):
            bits(ua[p], ub[p], "after two more ticks, pop %d" % p)
    finally:
        pl.close()
        twin.close()


def _where(msg):
    m = re.search(r"population (\d+), point (\d+), obstacle (\d+), component (\d+)", msg)
    assert m, msg
    return tuple(int(v) for v in m.groups())


@pytest.mark.parametrize("dtype,c", tref.PAIRS, ids=lambda v: str(v))
def test_validation_names_the_first_offender_and_changes_nothing(pmaf, scenes, torch, dtype, c):
    scs = [scenes.synthetic_scene(sref.N_AGENTS, 8, tref.VALID_M, config_id=11, scene_id=p, dynamic=False) for p in range(2)]
    assert scs[0]["dt"] == tref.DT
    pl = planner(pmaf, scs)
    try:
        good = tref.validation_source(dtype, c)       # NaN and 1e35 in its padding
        pl.set_obstacle_tracks_device(dev(torch, good), tref.VALID_LEN)
        pl.set_obstacle_track_offset([1, 2])
        base = [tref.expected_tracks(good[p, :tref.VALID_LEN[p]], c, tref.DT) for p in range(2)]
        ref = roll(pl)
        cfg = pl.launch_config()

        def unchanged(tag):
            used, first = pl.get_obstacle_tracks()
            for p in range(2):
                bits(used[p], base[p], tag)
            assert list(first) == [1, 2] and pl.launch_config() == cfg
            same(roll(pl), ref, tag)

        cases = [k for k in tref.validation_cases() if (k[0], k[1]) == (dtype, c)]
        assert len(cases) >= 16
        for _, _, vname, pname, s, want in cases:
            msg = _raises(ERR_INVALID, pl.set_obstacle_tracks_device, dev(torch, s), tref.VALID_LEN)
            assert _where(msg) == want, (vname, pname, msg)
            unchanged("%s at %s" % (vname, pname))
        s, want = tref.two_bad(dtype, c)
        assert _where(_raises(ERR_INVALID, pl.set_obstacle_tracks_device, dev(torch, s), tref.VALID_LEN)) == want
        unchanged("two bad values")
        # arguments
        t = dev(torch, good)
        _raises(ERR_INVALID, pl.set_obstacle_tracks_device, t, [tref.VALID_MAX + 1, 1])
        _raises(ERR_INVALID, pl.set_obstacle_tracks_device, t, [2, -1])
        kw = dict(dtype=dtype.replace("f", "float"), max_len=tref.VALID_MAX)
        _raises(ERR_INVALID, pl.set_obstacle_tracks_device, t.data_ptr(), tref.VALID_LEN, components=4, **kw)
        _raises(ERR_INVALID, pl.set_obstacle_tracks_device, t.data_ptr(), tref.VALID_LEN, components=c, dtype=7, max_len=tref.VALID_MAX)
        _raises(ERR_INVALID, pl.set_obstacle_tracks_device, t.data_ptr(), tref.VALID_LEN, components=c, dtype=kw["dtype"], max_len=0)
        _raises(ERR_INVALID, pl.set_obstacle_tracks_device, 0, tref.VALID_LEN, components=c, **kw)                   # d_tracks == NULL
        # misaligned by two bytes: refused by the host's alignment check, nothing is enqueued. (The extent that WOULD be read
        # -- the lengths lie two points short of max_len -- stays inside the tensor's allocation, and the pointer is the
        # tensor's own memory: this is an argument refusal, not a pointer the device cannot read.)
        _raises(ERR_INVALID, pl.set_obstacle_tracks_device, t.data_ptr() + 2, tref.VALID_LEN, components=c, **kw)
        import ctypes as C
        assert pl.L.pmaf_set_obstacle_tracks_device(pl._h, C.c_void_p(t.data_ptr()), None, tref.VALID_MAX, c,
                                                    pl._track_dtype(kw["dtype"]), None) == ERR_INVALID                # len == NULL
        unchanged("after the argument refusals")
    finally:
        pl.close()


def test_unsupported_routes_refuse_with_the_host_calls_message(pmaf, scenes, torch):
    sc = scenes.synthetic_scene(sref.N_AGENTS, 8, 61, config_id=11)
    pl = planner(pmaf, sc)
    try:
        n0 = pl.launch_count()
        t = dev(torch, tref.make_source(61, 2, 3, "f32"))
        msg = _raises(ERR_STATE, pl.set_obstacle_tracks_device, t)
        host = _raises(ERR_STATE, pl.set_obstacle_tracks, np.zeros((2, 61, 6)) + 0.5)
        assert "obstacle tracks" in msg and ("multi-wave" in msg or "slots" in msg), msg
        assert msg.split(":", 2)[2] == host.split(":", 2)[2]
        assert pl.launch_count() == n0 and [len(x) for x in pl.get_obstacle_tracks()[0]] == [0]
        pl.rollout()
        assert pl.launch_count() == n0 + 1
    finally:
        pl.close()
    sc = scene_for(scenes, "M3-cap9")
    pl = planner(pmaf, sc, contracted=True)
    try:
        n0 = pl.launch_count()
        msg = _raises(ERR_STATE, pl.set_obstacle_tracks_device, dev(torch, tref.make_source(3, 2, 6, "f64")))
        assert "obstacle tracks" in msg and "policy" in msg, msg
        assert pl.launch_count() == n0 and [len(x) for x in pl.get_obstacle_tracks()[0]] == [0]
    finally:
        pl.close()


def test_ingest_waits_for_the_producer_stream_and_copies(pmaf, scenes, torch):
    sc = scene_for(scenes, "M59-cap70-moving")
    pl, twin = planner(pmaf, sc), planner(pmaf, sc)
    try:
        final = tref.parity_source("M59-cap70-moving", "f32", 3)
        other = tref.make_source(59, 70, 3, "f32", seed=41)
        want = tref.expected_tracks(final, 3, sc["dt"])
        src, fin = dev(torch, other), dev(torch, final)
        big = torch.ones(96 * 1024 * 1024, dtype=torch.float32, device="cuda:0")     # 384 MB
        side = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(24):                # some 10 ms of elementwise passes in front of the fill, not synchronised
                big.mul_(1.0001)
            src.copy_(fin)
        pending = not side.query()
        pl.set_obstacle_tracks_device(src, producer_stream=side.cuda_stream)
        print("the fill was still pending when the call was made:", pending)
        assert pending
        bits(pl.get_obstacle_tracks()[0][0], want, "the final values")
        # the source may be overwritten on return: the next rollout follows the ingested values
        src.copy_(dev(torch, other))
        torch.cuda.synchronize()
        twin.set_obstacle_tracks(want)
        same(roll(pl), roll(twin), "after the source was overwritten")
        bits(pl.get_obstacle_tracks()[0][0], want, "still the ingested values")
    finally:
        pl.close()
        twin.close()


def test_closed_loop_fresh_tensor_every_tick(pmaf, scenes, torch):
    """five six-call ticks, a fresh F32 / 3 device tensor in front of each start, the selection
    select_clear_tracked(adopt=1): picks, set-points and clearances equal a twin fed through the host call"""
    sc = scene_for(scenes, "M3-cap70")
    cap = sc["max_prediction_steps"]
    pl, twin = planner(pmaf, sc), planner(pmaf, sc)
    try:
        for h in (pl, twin):
            h.start()
        for t in range(5):
            src = tref.make_source(3, cap, 3, "f32", seed=50 + t)
            want = tref.expected_tracks(src, 3, sc["dt"])
            row = []
            for h in (pl, twin):
                h.stop()
                h.evaluate(sc["cost_gains"], sc["ws_limits"])
                sel = h.select_clear_tracked(sc["obstacles"], 0.0, cap, adopt=True)
                h.move_real(sc["obstacles"], sc["dt"], 1, sel["pick"])
                pos, vel, _ = h.real_state()
                h.reset_agents(pos, vel, sc["obstacles"])
                if h is pl:
                    h.set_obstacle_tracks_device(dev(torch, src))
                else:
                    h.set_obstacle_tracks(want)
                h.start()
                row.append((sel, np.asarray(pos).copy()))
            (sa, pa), (sb, pb) = row
            assert sorted(sa) == sorted(sb)
            for k in sa:
                np.testing.assert_array_equal(np.asarray(sa[k]), np.asarray(sb[k]), err_msg="tick %d %s" % (t, k))
            np.testing.assert_array_equal(pa, pb, err_msg="tick %d set-point" % t)
        for h in (pl, twin):
            h.stop()
        bits(pl.get_obstacle_tracks()[0][0], twin.get_obstacle_tracks()[0][0], "the last tick's tracks")
    finally:
        pl.close()
        twin.close()


def test_facade_set_obstacle_tracks_device(pmaf, scenes, tmp_path):
    """tests/cpp/facade_device_tracks.cpp: hipMalloc, copy, CfManager::setObstacleTracksDevice (offset 2), advances, a
    second shorter attach, a detach; every figure it prints equals the same calls made through the binding"""
    import conftest
    torch = pytest.importorskip("torch")
    N, cap, ticks, L = 12, 101, 6, 40
    sc = scenes.static1_scene(N, cap - 1)
    rvf = tmp_path / "rv.bin"
    np.ascontiguousarray(sc["random_vecs"]).tofile(rvf)
    exe = conftest.exe(os.path.join(conftest.ROOT, "tests", "cpp", "facade_device_tracks"))
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    out = subprocess.run([exe, str(N), str(cap), str(ticks), str(rvf), str(L)], capture_output=True, check=True,
                         env=conftest.binary_env(pmaf)).stdout.decode()
    lines = out.strip().split("\n")
    assert len(lines) == ticks
    k = np.arange(L, dtype=np.float64)
    x = np.zeros((L, 9, 3))
    x[:] = sc["obstacles"][None, :9, 0:3]
    x[:, :, 0] = sc["obstacles"][None, :9, 0] + 0.0005 * k[:, None]
    x[:, 0] = np.stack([-0.6 + 0.002 * k, 0.3 - 0.001 * k, np.full(L, 0.75)], axis=1)
    t = dev(torch, x.astype(np.float32))
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    plain = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        differs = False
        for h in (pl, plain):
            h.set_initial_position(sc["start"])
            h.start()
        for tick in range(ticks):
            if tick == 0:
                pl.set_obstacle_tracks_device(t)
                pl.set_obstacle_track_offset(2)
            elif tick + 2 < ticks:
                pl.set_obstacle_track_offset(2 + tick)
            elif tick + 2 == ticks:
                pl.set_obstacle_tracks_device(t, [L // 2])
            else:
                pl.set_obstacle_tracks_device(t, [0])
            row = []
            for h in (pl, plain):
                b = h.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
                h.stop()
                paths, n = h.paths()
                row.append((b, int(n[b]), h.last_next_pos[0].copy(), paths[b, n[b] - 1].copy()))
            f = lines[tick].split()
            b, nb, nxt, end = row[0]
            assert [int(v) for v in f[:3]] == [tick, b, nb]
            np.testing.assert_array_equal(np.array(f[3:6], dtype=float), nxt)
            np.testing.assert_array_equal(np.array(f[6:9], dtype=float), end)
            differs = differs or not np.array_equal(end, row[1][3])
        assert differs
    finally:
        pl.close()
        plain.close()
