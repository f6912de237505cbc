"""The two step loops of the one-slot DPP sum on the GPU (csrc/pmaf_rollout_w64_body.hpp: the short loop until the first
step with more than 16 terms, the long loop -- second chunk added in the block of the scaling chain, whatever the count --
from the next step on), bit for bit against the CPU oracle. The scenes of tests/long_loop_scenes.py change K along one
rollout: short -> long -> short (K = 3 right behind K = 25: a stale second chunk must not be added) -> nothing inside
the shell -> long again up to the capacity's last step; a long first step, then K = 16, 17, 33, 32, 16 inside the long
loop. Field obstacles at rest, a cluster flying head-on / a far mover (the bodies that advance), the repulsive obstacle
far and in range (lane 60); the same with a repulsive track (csrc/pmaf_k_track.hip), with obstacle tracks
(pmaf_k_ftrack.hip) and at 1.5 waves per SIMD (k_rollout_w64_sliced). Every case: three ticks; best index, set-point
(the real agent's position and velocity), paths, point counts, costs, rotation vectors and min_obs_dist of every tick.
tests/test_long_loop.py checks on the CPU that the scenes hold the K sequences they claim: without it this module
could pass on scenes that never leave the short loop. It pins behaviour: a library with one step loop passes it too."""
import numpy as np
import pytest

import field_track_reference as fref
import long_loop_scenes as lls
import sentinel_track_reference as sref

pytestmark = pytest.mark.gpu

TICKS = 3
KEYS = ("real_pos", "real_vel", "paths", "n_points", "costs", "rot", "min_obs")


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("PMAF_SUM", "PMAF_FORCE_GENERIC", "PMAF_PLAIN_STEP", "PMAF_MW", "PMAF_W64_SLICE"):
        monkeypatch.delenv(k, raising=False)


def _state(pl):
    """what is compared after a tick"""
    pl.stop()
    paths, n = pl.paths()
    pos, vel, _ = pl.real_state()
    return dict(real_pos=pos, real_vel=vel, paths=paths, n_points=n, costs=pl.costs(), rot=pl.rot_vecs(),
                min_obs=pl.min_obs_dist())


_REF = {}


def reference(oracle, scenes, name, moving, sent_near, ftracks=None, track=None):
    """per tick (best index, results) of the oracle: computed once per case, shared, never modified. With tracks the
    rollout of a tick is the composed one of the track references (tests/sentinel_track_reference.py,
    tests/field_track_reference.py), as in tests/test_sum_chunks_gpu.py."""
    key = (name, moving, sent_near, ftracks is not None, track is not None)
    if key in _REF:
        return _REF[key]
    sc = lls.build_scene(scenes, name, moving, sent_near)
    ora = oracle.OraclePlanner(sc, mgr_init_pos=lls.INIT)
    lls.prepare(ora)
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
        pos, vel, _ = ora.real_state()
        res = dict(real_pos=np.array(pos), real_vel=np.array(vel), paths=paths.copy(), n_points=n.copy(), costs=ora.costs(),
                   rot=ora.rot_vecs(), min_obs=ora.min_obs_dist())
        assert (n == sc["max_prediction_steps"]).all()      # every rollout runs to the capacity
        ticks.append((best, res))
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
    pl = pmaf.PmafPlanner(scenes_arg, device=0, mgr_init_pos=np.tile(lls.INIT, (P, 1)), **(planner_kw or {}))
    try:
        pl.set_real_position(np.tile(lls.START, (P, 1)))
        cfg = pl.launch_config()
        assert cfg["lanes_per_agent"] == 64 and cfg["waves_per_agent"] == 1, cfg
        assert bool(cfg["priority_slices"]) == expect_sliced, cfg
        if setup is not None:
            setup(pl)
        obs = sc["obstacles"] if P == 1 else np.stack([sc["obstacles"]] * P)
        for t, (best, want) in enumerate(ticks):
            b = pl.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
            got = _state(pl)
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


@pytest.mark.parametrize("name,moving,sent_near", lls.cases())
def test_k_varies_three_ticks(pmaf, oracle, scenes, name, moving, sent_near):
    sc, ticks, costs = reference(oracle, scenes, name, moving, sent_near)
    run_and_compare(pmaf, sc, ticks, costs, tag="%s moving=%s sent=%s" % (name, moving, sent_near))


def _track(sc):
    """a repulsive track 0.6 m beside the agents' line, drifting along it: in repelForce's range at every step"""
    n = sc["max_prediction_steps"] + 2
    return (lls.START + np.array([1.0, 0.6, 0.0]))[None, :] + np.arange(n)[:, None] * np.array([0.3, -0.01, 0.005])[None, :]


@pytest.mark.parametrize("name", sorted(lls.SCENES))
def test_k_varies_with_a_repulsive_track(pmaf, oracle, scenes, name):
    """k_rollout_w64_track, the loop that carries the tracked repulsive obstacle in lane 60"""
    track = _track(lls.build_scene(scenes, name, False, True))
    sc, ticks, costs = reference(oracle, scenes, name, False, True, track=track)
    plain = reference(oracle, scenes, name, False, True)[1]
    assert not np.array_equal(ticks[-1][1]["paths"], plain[-1][1]["paths"])        # the track matters

    def setup(pl):
        pl.set_repulsive_track(track)
    run_and_compare(pmaf, sc, ticks, costs, setup=setup, tag="%s repulsive track" % name)


def _obstacle_tracks(sc0):
    """a track per field obstacle, 2 mm beside its live position and drifting 0.5 mm per point"""
    ft = fref.straight_lines(sc0["obstacles"], sc0["dt"], sc0["max_prediction_steps"] + 2)
    ft[:, :, 0:3] += np.array([0.0, 0.002, -0.001])[None, None, :] + np.arange(len(ft))[:, None, None] * 0.0005
    return ft


@pytest.mark.parametrize("name", sorted(lls.SCENES))
def test_k_varies_with_obstacle_tracks(pmaf, oracle, scenes, name):
    """every field obstacle follows a track 2 mm beside its live position, drifting 0.5 mm per point: far inside the
    scenes' margins, K stays what it is (k_rollout_w64_ftrack)"""
    ft = _obstacle_tracks(lls.build_scene(scenes, name, False, False))
    sc, ticks, costs = reference(oracle, scenes, name, False, False, ftracks=ft)
    plain = reference(oracle, scenes, name, False, False)[1]
    assert not np.array_equal(ticks[-1][1]["paths"], plain[-1][1]["paths"])        # the tracks matter

    def setup(pl):
        pl.set_obstacle_tracks(ft)
    run_and_compare(pmaf, sc, ticks, costs, setup=setup, tag="%s obstacle tracks" % name)


@pytest.mark.parametrize("name", sorted(lls.SCENES))
def test_k_varies_at_one_and_a_half_waves_per_simd(pmaf, oracle, scenes, name):
    """220 populations of the seven agents: 1 540 waves on 1 024 SIMDs, the priority-sliced kernel; every population
    rolls the same scene out and must hand back the oracle's bits"""
    sc, ticks, costs = reference(oracle, scenes, name, False, False)
    run_and_compare(pmaf, sc, ticks, costs, P=220, expect_sliced=True, tag="%s sliced" % name)
