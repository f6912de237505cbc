"""The host side's grown-on-demand scratch (csrc/pmaf_host_impl.hpp: DeviceBuf / PinnedBuf) at TOLERANCE 0: one handle
runs a sequence of calls in which every scratch area -- the path audit's, the cross audit's, the link force's, the
repulsive track's -- has to GROW AFTER IT HAS BEEN USED, and every result must equal, bit for bit, the same single call
on a fresh handle brought to the same state (rollouts are deterministic, so the fresh handle's paths are identical).

The sizes below restate the host's sizing rules (pmaf_host_audit.cpp: evaluate_paths, xaudit_scratch, pmaf_link_force;
pmaf_host.cpp: upload_tracks) from the shapes of this test, and the test asserts that the sequence really contains, for
each area, a call that needs more bytes than every earlier one: shortened later, it fails instead of passing vacuously.
The link force's buffer never holds fewer than 512 doubles, so the issue's n = 1, 9 only grow it from empty; n = 80
(567 doubles) is added to make it grow after use as well."""
import numpy as np
import pytest

from test_path_audit_gpu import _same_bits, live_list, rollout_case

pytestmark = pytest.mark.gpu

P, N, M, H = 2, 5, 2, 8          # n_obs = M + 1 = 3, cap = H + 1 = 9
SEP, MARGIN = 0.15, 0.06
# csrc/pmaf_types.hpp: sizeof(PairBest), sizeof(PairResult), sizeof(PairClearBest), PMAF_XAUDIT_PARTIALS
PAIR_BEST, PAIR_RESULT, PAIRCLEAR_BEST, PARTIALS = 24, 32, 32, 256


def _pad8(b):
    return (b + 7) & ~7


def audit_bytes(cap, n_obs, per_obstacle):
    full = P * N
    return 8 * P * cap * 3 * n_obs + 8 * full + (8 * full * n_obs if per_obstacle else 0) + 3 * 4 * full


def xaudit_bytes(cap, n_a, n_b, n_tracks, two_steps, joint):
    pairs = n_a * n_b
    b_step = _pad8(4 * pairs)
    total = 8 * pairs + PAIR_BEST * PARTIALS + PAIR_RESULT + 8 * n_tracks * cap * 3 + b_step + _pad8(4 * n_tracks)
    total += b_step if two_steps else 0
    total += (PAIRCLEAR_BEST * PARTIALS + 8 * n_tracks + _pad8(4 * n_a) + _pad8(4 * n_b)) if joint else 0
    return total


def link_doubles_needed(n):
    return 7 * n + 7


def link_doubles_held(held, n):
    need = link_doubles_needed(n)
    return held if need <= held else (512 if need < 512 else 2 * need)


def track_bytes(cap, max_len):
    return 8 * P * min(max_len, cap) * 3


def _same(got, want, what):
    if isinstance(got, dict):
        assert sorted(got) == sorted(want), what
        for k in got:
            _same(got[k], want[k], "%s[%s]" % (what, k))
    elif isinstance(got, (tuple, list)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s[%d]" % (what, i))
    else:
        g = np.asarray(got)
        assert g.shape == np.asarray(want).shape, what
        _same_bits(g.astype(np.float64), np.asarray(want, dtype=np.float64), what)   # (int32 values convert exactly)


def _handle(pmaf, scenes):
    """the state every call of the sequence starts from: one rollout, one evaluate"""
    pl, scs, start = rollout_case(pmaf, scenes, P, N, M, H)
    pl.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
    return pl, live_list(scenes, start)


def _grows_after_use(sizes, what):
    """some call needs more than every earlier call of a non-empty prefix"""
    assert any(sizes[i] > max(sizes[:i]) for i in range(1, len(sizes))), "%s: no call outgrows the earlier ones: %s" % (what, sizes)


def test_every_scratch_area_grows_after_use_and_serves_the_same_results(pmaf, scenes):
    used, live = _handle(pmaf, scenes)
    cap = used.cap
    assert (used.P, used.N, used.n_obs, cap) == (P, N, M + 1, H + 1)
    rng = np.random.default_rng(11)

    def tracks(n):
        t = rng.uniform(-1.0, 1.0, (n, cap, 3))
        t[:, :, 2] += 0.7
        return t, np.asarray(([1, cap // 2, cap] * n)[:n], dtype=np.int32)

    tr1, tr70, tr3 = tracks(1), tracks(70), tracks(3)     # 70: past one 64-lane tile
    cost70 = rng.uniform(0.0, 2.0, 70)

    def link(n):
        return rng.uniform(-1.0, 1.0, (n, 3)), rng.uniform(0.1, 2.0, n)

    lk1, lk9, lk80 = link(1), link(9), link(80)
    rp2 = [np.array([[0.1, 0.2, 0.7], [0.15, 0.2, 0.7]]), np.array([[-0.1, 0.3, 0.6], [-0.1, 0.35, 0.6]])]
    rp8 = [np.linspace([0.1, 0.2, 0.7], [0.5, 0.1, 0.6], 8), np.linspace([-0.1, 0.3, 0.6], [-0.4, 0.2, 0.8], 8)]

    def track_roundtrip(pl, t):
        pl.set_repulsive_track(t)
        return pl.get_repulsive_track()

    # (name, the call, the scratch area it uses, the bytes / doubles it needs there)
    calls = [
        ("evaluate_path", lambda pl: pl.evaluate_path(live), "audit", audit_bytes(cap, M + 1, False)),
        ("evaluate_paths", lambda pl: pl.evaluate_paths(live, MARGIN), "audit", audit_bytes(cap, M + 1, False)),
        ("evaluate_paths per_obstacle", lambda pl: pl.evaluate_paths(live, MARGIN, per_obstacle=True), "audit",
         audit_bytes(cap, M + 1, True)),
        ("cross_audit_tracks 1", lambda pl: pl.cross_audit_tracks(0, tr1[0], tr1[1], SEP, step=True), "xaudit",
         xaudit_bytes(cap, N, 1, 1, False, False)),
        ("cross_audit_tracks 70", lambda pl: pl.cross_audit_tracks(0, tr70[0], tr70[1], SEP, step=True), "xaudit",
         xaudit_bytes(cap, N, 70, 70, False, False)),
        ("cross_audit_tracks 3", lambda pl: pl.cross_audit_tracks(1, tr3[0], tr3[1], SEP, step=True), "xaudit",
         xaudit_bytes(cap, N, 3, 3, False, False)),
        ("cross_audit_tracks_slack 70", lambda pl: pl.cross_audit_tracks_slack(0, tr70[0], tr70[1], SEP, 2, 1, steps=True),
         "xaudit", xaudit_bytes(cap, N, 70, 70, True, False)),
        ("select_clear_tracks 70", lambda pl: pl.select_clear_tracks(0, live, MARGIN, H, tr70[0], tr70[1], SEP, 0.01,
                                                                     track_cost=cost70), "xaudit",
         xaudit_bytes(cap, N, 70, 70, False, True)),
        ("select_pair_clear", lambda pl: pl.select_pair_clear(0, 1, live, MARGIN, H, SEP, 0.01), "xaudit",
         xaudit_bytes(cap, N, N, 0, False, True)),
        ("link_force 1", lambda pl: pl.link_force(lk1[0], lk1[1], live, pop=0), "link", link_doubles_needed(1)),
        ("link_force 9", lambda pl: pl.link_force(lk9[0], lk9[1], live, pop=1), "link", link_doubles_needed(9)),
        ("link_force 80", lambda pl: pl.link_force(lk80[0], lk80[1], live, pop=0), "link", link_doubles_needed(80)),
        ("repulsive track 2", lambda pl: track_roundtrip(pl, rp2), "track", track_bytes(cap, 2)),
        ("repulsive track 8", lambda pl: track_roundtrip(pl, rp8), "track", track_bytes(cap, 8)),
    ]
    for area in ("audit", "xaudit", "link", "track"):
        sizes = [c[3] for c in calls if c[2] == area]
        print(area, sizes)
        _grows_after_use(sizes, area)
    # the link buffer's floor: what it HOLDS must grow after use too (n = 80), not only what a call needs
    held = [0]
    for n in (1, 9, 80):
        held.append(link_doubles_held(held[-1], n))
    print("link doubles held", held[1:])
    _grows_after_use(held[1:], "link (held)")

    try:
        got = [(name, fn(used)) for name, fn, _, _ in calls]
    finally:
        used.close()
    for (name, g), (_, fn, _, _) in zip(got, calls):
        fresh, _ = _handle(pmaf, scenes)
        try:
            want = fn(fresh)
        finally:
            fresh.close()
        _same(g, want, name)
    # the two tracks came back as given (the round trip itself, not only used == fresh)
    _same(dict(got)["repulsive track 2"], rp2, "track 2 as given")
    _same(dict(got)["repulsive track 8"], rp8, "track 8 as given")
