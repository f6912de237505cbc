"""The one-slot DPP sum's chunks on the GPU (csrc/pmaf_rollout_w64.hpp, circ_and_scale_w64: first chunk in the block of
the scaling chain, the second out of the registers it was prefetched into, further ones in the prefetching loop), bit for
bit against the CPU oracle. The scenes of tests/sum_chunk_scenes.py hold K terms in the list at every step: K runs over
both sides of the chunk boundaries 16, 32 and 48 and up to the full 60, with the field obstacles at rest and with one
moving (the bodies that assume rest / that advance), with the repulsive obstacle far and in range. K = 17 and 33 also
run on a handle with a repulsive track (csrc/pmaf_k_track.hip), one with obstacle tracks (pmaf_k_ftrack.hip) and at
1.5 waves per SIMD (k_rollout_w64_sliced). Every case: three ticks; paths, point counts, costs, rotation vectors and
min_obs_dist of every tick. tests/test_sum_chunks.py checks on the CPU that the scenes hold the K they claim."""
import numpy as np
import pytest

import field_track_reference as fref
import sentinel_track_reference as sref
import sum_chunk_scenes as scs

pytestmark = pytest.mark.gpu

TICKS = 3
KEYS = ("paths", "n_points", "costs", "rot", "min_obs")     # costs right after a tick: those its selection read


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("PMAF_SUM", "PMAF_FORCE_GENERIC", "PMAF_PLAIN_STEP", "PMAF_MW", "PMAF_W64_SLICE"):
        monkeypatch.delenv(k, raising=False)


def _state(pl, sc):
    """what is compared after a tick"""
    pl.stop()
    paths, n = pl.paths()
    return dict(paths=paths, n_points=n, costs=pl.costs(), rot=pl.rot_vecs(), min_obs=pl.min_obs_dist())


_REF = {}


def reference(oracle, scenes, K, moving, sent_near, ftracks=None, track=None, edit=None):
    """per tick (best index, results) of the oracle: computed once per case, shared, never modified. With tracks the
    rollout of a tick is the composed one of the track references (select, real step against the live list, reset,
    rollout against the tracks: tests/sentinel_track_reference.py coupled_ticks, tests/field_track_reference.py
    tracked_ticks). edit: (tag, function) -- the scene is function(scene) (other dynamics on the same obstacles:
    tests/variant_matrix.py general_scene), the reference its own."""
    key = (K, moving, sent_near, ftracks is not None, track is not None, edit[0] if edit else None)
    if key in _REF:
        return _REF[key]
    sc = scs.build_scene(scenes, K, moving, sent_near)
    if edit:
        sc = edit[1](sc)
    ora = oracle.OraclePlanner(sc, mgr_init_pos=scs.INIT)
    scs.prepare(ora)
    ticks = []
    for t in range(TICKS):
        if ftracks is None and track is None:
            best = ora.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
        else:
            best = ora.evaluate(sc["cost_gains"], sc["ws_limits"])
            ora.move_real(sc["obstacles"], sc["dt"], 1, best)
            pos, vel, _ = ora.real_state()
            ora.reset_agents(pos, vel, sc["obstacles"])
            if ftracks is not None:
                fref.compose(ora, oracle.eval_order(), sc, sc["obstacles"], ftracks, 0)
            else:
                sref.compose(ora, oracle.eval_order(), sc, sc["obstacles"], track)
        paths, n = ora.paths()
        res = dict(paths=paths.copy(), n_points=n.copy(), costs=ora.costs(), rot=ora.rot_vecs(), min_obs=ora.min_obs_dist())
        if t == 0:     # the construction, once more where the kernels run: K terms at the first step
            pos, vel, _ = ora.real_state()
            assert scs.terms_at(sc, pos, vel, scs.INIT) == scs.holders(K)
        ticks.append((best, res))
    # the last rollout's costs (pmaf_evaluate / orc_evaluate on the paths as they lie)
    ora.evaluate(sc["cost_gains"], sc["ws_limits"])
    final_costs = ora.costs()
    ora.close()
    for _, r in ticks:
        for v in r.values():
            v.setflags(write=False)
    _REF[key] = (sc, ticks, final_costs)
    return _REF[key]


def run_and_compare(pmaf, sc, ticks, final_costs, P=1, setup=None, expect_sliced=False, tag="", planner_kw=None):
    """planner_kw: further keyword arguments of PmafPlanner (the arithmetic policy: tests/variant_matrix.py)"""
    scenes_arg = sc if P == 1 else [sc] * P
    pl = pmaf.PmafPlanner(scenes_arg, device=0, mgr_init_pos=np.tile(scs.INIT, (P, 1)), **(planner_kw or {}))
    try:
        pl.set_real_position(np.tile(scs.START, (P, 1)))
        cfg = pl.launch_config()
        assert cfg["lanes_per_agent"] == 64 and cfg["waves_per_agent"] == 1, cfg
        assert bool(cfg["priority_slices"]) == expect_sliced, cfg
        if setup is not None:
            setup(pl)
        obs = sc["obstacles"] if P == 1 else np.stack([sc["obstacles"]] * P)
        for t, (best, want) in enumerate(ticks):
            b = pl.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
            got = _state(pl, sc)
            np.testing.assert_array_equal(np.asarray(b).reshape(P), np.full(P, best), err_msg="%s tick %d best" % (tag, t))
            for k in KEYS:
                g = np.asarray(got[k]).reshape((P,) + np.asarray(want[k]).shape)
                bad = int((g != np.asarray(want[k])[None]).sum())
                print("%s tick %d %s: %d differing entries" % (tag, t, k, bad))
                np.testing.assert_array_equal(g, np.broadcast_to(np.asarray(want[k])[None], g.shape), err_msg="%s tick %d %s" % (tag, t, k))
        pl.evaluate(sc["cost_gains"], sc["ws_limits"])
        c = np.asarray(pl.costs()).reshape(P, -1)
        np.testing.assert_array_equal(c, np.broadcast_to(final_costs[None], c.shape), err_msg="%s costs" % tag)
    finally:
        pl.close()


@pytest.mark.parametrize("K,moving,sent_near", scs.cases())
def test_k_terms_three_ticks(pmaf, oracle, scenes, K, moving, sent_near):
    sc, ticks, costs = reference(oracle, scenes, K, moving, sent_near)
    run_and_compare(pmaf, sc, ticks, costs, tag="K%d moving=%s sent=%s" % (K, moving, sent_near))


def _track():
    return scs.START[None, :] + np.array([-0.05, 0.3, 0.0])[None, :] + np.arange(scs.CAP + 2)[:, None] * np.array([0.004, -0.002, 0.001])[None, :]


def _obstacle_tracks(sc0):
    ft = fref.straight_lines(sc0["obstacles"], sc0["dt"], scs.CAP + 2)
    ft[:, :, 0:3] += np.array([0.0, 0.002, -0.001])[None, None, :] + np.arange(len(ft))[:, None, None] * 0.0005
    return ft


@pytest.mark.parametrize("K", scs.TRACK_KS)
def test_k_terms_with_a_repulsive_track(pmaf, oracle, scenes, K):
    """the tracked repulsive obstacle passes 0.3 m beside the agents, in repelForce's range (k_rollout_w64_track)"""
    track = _track()
    sc, ticks, costs = reference(oracle, scenes, K, False, True, track=track)
    plain = reference(oracle, scenes, K, False, True)[1]
    assert not np.array_equal(ticks[-1][1]["paths"], plain[-1][1]["paths"])        # the track matters

    def setup(pl):
        pl.set_repulsive_track(track)
    run_and_compare(pmaf, sc, ticks, costs, setup=setup, tag="K%d repulsive track" % K)


@pytest.mark.parametrize("K", scs.TRACK_KS)
def test_k_terms_with_obstacle_tracks(pmaf, oracle, scenes, K):
    """every field obstacle follows a track 2 mm beside its live position, drifting (k_rollout_w64_ftrack)"""
    ft = _obstacle_tracks(scs.build_scene(scenes, K, False, False))
    sc, ticks, costs = reference(oracle, scenes, K, False, False, ftracks=ft)
    plain = reference(oracle, scenes, K, False, False)[1]
    assert not np.array_equal(ticks[-1][1]["paths"], plain[-1][1]["paths"])        # the tracks matter

    def setup(pl):
        pl.set_obstacle_tracks(ft)
    run_and_compare(pmaf, sc, ticks, costs, setup=setup, tag="K%d obstacle tracks" % K)


@pytest.mark.parametrize("K", scs.TRACK_KS)
def test_k_terms_at_one_and_a_half_waves_per_simd(pmaf, oracle, scenes, K):
    """220 populations of the seven agents: 1 540 waves on 1 024 SIMDs, the priority-sliced kernel; every population
    rolls the same scene out and must hand back the oracle's bits"""
    sc, ticks, costs = reference(oracle, scenes, K, False, False)
    run_and_compare(pmaf, sc, ticks, costs, P=220, expect_sliced=True, tag="K%d sliced" % K)
