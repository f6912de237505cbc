"""The scenes of tests/sum_chunk_scenes.py on the CPU oracle: every case has the intended number K of terms in the
ordered force sum at the first step of its first rollout -- counted by geometry on the oracle's own start state (the
first path point and the velocity the agents were reset to) -- and keeps it, with the builder's margin to spare, at
every path point of three ticks. No GPU."""
import numpy as np
import pytest

import sum_chunk_scenes as scs
import variant_matrix as vm


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


def _placement(sc, K):
    """the builder's promise, on the scene alone: K obstacles >= MARGIN inside the shell round the start, in front of
    the agent, the others >= MARGIN outside"""
    g = (sc["goal"] - sc["start"]) / np.linalg.norm(sc["goal"] - sc["start"])
    inside = []
    for i, o in enumerate(sc["obstacles"][:-1]):
        d = np.linalg.norm(o[0:3] - sc["start"]) - (sc["radius"] + o[6])
        assert d <= sc["detect_shell_rad"] - scs.MARGIN or d >= sc["detect_shell_rad"] + scs.MARGIN, (i, d)
        if d < sc["detect_shell_rad"]:
            assert d >= 0.05 and np.dot(o[0:3] - sc["start"], g) > 0.0, (i, d)
            assert not o[3:6].any() or K == scs.M      # (K = M: the mover is a holder, see build_scene)
            inside.append(i)
    assert inside == scs.holders(K) and len(inside) == K
    assert np.linalg.norm(scs.INIT - sc["start"]) >= 0.2


@pytest.mark.parametrize("K,moving,sent_near", scs.cases())
def test_first_step_has_k_terms(oracle, scenes, K, moving, sent_near):
    _holds_k(oracle, scs.build_scene(scenes, K, moving, sent_near), K, moving, sent_near)


@pytest.mark.parametrize("variant", vm.GENERAL_VARIANTS)
@pytest.mark.parametrize("moving,sent_near", vm.SUM_CHUNK_STRICT_FLAGS)
@pytest.mark.parametrize("K", vm.GENERAL_KS)
def test_k_is_held_with_inputs_that_need_the_general_step(oracle, scenes, K, moving, sent_near, variant):
    """agent_mass = 2.5, and k_attr = 0 for agents 1 and 4 on top (tests/variant_matrix.py general_scene): other
    dynamics on the same obstacles -- the margins still hold K at every step of every tick"""
    sc = vm.general_scene(scs.build_scene(scenes, K, moving, sent_near), variant)
    assert sc["agent_mass"] == 2.5 and (np.ndim(sc["k_attr"]) == 1) == (variant == "mass_noattr")
    _holds_k(oracle, sc, K, moving, sent_near)


def _holds_k(oracle, sc, K, moving, sent_near):
    assert sc["obstacles"].shape == (scs.M + 1, 7) and sc["n_agents"] == scs.N_AGENTS == 7
    assert sorted(set(sc["agent_types"].tolist())) == [1, 2, 3, 4, 5, 6] and (sc["agent_types"] == 5).sum() == 2
    assert bool(sc["obstacles"][:-1, 3:6].any()) == moving
    sent_d = np.linalg.norm(sc["obstacles"][-1, 0:3] - sc["start"]) - (sc["radius"] + sc["obstacles"][-1, 6])
    assert (sent_d < sc["detect_shell_rad"] - scs.MARGIN) == sent_near
    _placement(sc, K)
    ora = oracle.OraclePlanner(sc, mgr_init_pos=scs.INIT)
    scs.prepare(ora)
    for t in range(3):
        ora.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
        pos, vel, _ = ora.real_state()        # what the agents were reset to: the rollouts' start state
        paths, n = ora.paths()
        assert (n == scs.CAP).all()
        for a in range(sc["n_agents"]):
            np.testing.assert_array_equal(paths[a, 0], pos)
        if t == 0:
            assert np.linalg.norm(vel) > 0.0
            first = scs.terms_at(sc, pos, vel, scs.INIT)
            assert first == scs.holders(K), (K, first)
            assert scs.terms_at(sc, pos, vel, scs.INIT, margin=0.04) == first      # and not by a hair
        # every later step: the same K (velocities from path differences; the margin covers what that leaves open)
        for a in range(sc["n_agents"]):
            for k in range(1, scs.CAP - 1):
                v = (paths[a, k] - paths[a, k - 1]) / sc["dt"]
                assert len(scs.terms_at(sc, paths[a, k], v, scs.INIT)) == K, (t, a, k)
                assert len(scs.terms_at(sc, paths[a, k], v, scs.INIT, margin=0.02)) == K, (t, a, k)
    ora.close()
