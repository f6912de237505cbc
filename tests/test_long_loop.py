"""The scenes of tests/long_loop_scenes.py on the CPU oracle: K, the number of terms in the ordered force sum, takes along
every rollout of three ticks exactly the sequence the builder promises (long_loop_scenes.k_at), for every agent -- one of
each heuristic and a second Random -- counted by geometry with the obstacles 0.05 m nearer and 0.05 m farther than they
are (sum_chunk_scenes.terms_at with the margin: both give the same K at every step). On those sequences the module then
asserts what tests/test_long_loop_gpu.py needs from them: the two step loops of the one-slot DPP sum
(csrc/pmaf_rollout_w64_body.hpp) are both run, and the long one meets the stale second chunk, an empty shell, the chunk
boundaries 16 / 17 and 32 / 33 and the capacity. No GPU."""
import numpy as np
import pytest

import long_loop_scenes as lls
import sum_chunk_scenes as scs

TICKS = 3


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


def k_sequences(oracle, sc, name, moving):
    """[tick][agent] -> K per step, asserted equal to the builder's promise and insensitive to the margin"""
    ora = oracle.OraclePlanner(sc, mgr_init_pos=lls.INIT)
    lls.prepare(ora)
    out = []
    for t in range(TICKS):
        ora.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
        pos, vel, _ = ora.real_state()
        paths, n = ora.paths()
        assert (n == sc["max_prediction_steps"]).all()
        want = [lls.k_at(name, t + k, moving, t) for k in range(sc["max_prediction_steps"] - 1)]
        per_agent = []
        for a in range(sc["n_agents"]):
            np.testing.assert_array_equal(paths[a, 0], pos)
            ks = []
            for k in range(int(n[a]) - 1):
                v = vel if k == 0 else (paths[a, k] - paths[a, k - 1]) / sc["dt"]
                at = dict(sc, obstacles=sc["obstacles"].copy())
                at["obstacles"][:, 0:3] += k * sc["dt"] * sc["obstacles"][:, 3:6]        # predictObstacles, k times
                K = len(scs.terms_at(at, paths[a, k], v, lls.INIT))
                assert K == len(scs.terms_at(at, paths[a, k], v, lls.INIT, margin=lls.MARGIN)), (t, a, k)
                assert K == len(scs.terms_at(at, paths[a, k], v, lls.INIT, margin=-lls.MARGIN)), (t, a, k)
                # the agents stay on the builder's lattice (what the margins were worked out for)
                assert abs(paths[a, k, 0] - lls.lattice(t + k)) < 0.02 and np.linalg.norm(paths[a, k, 1:] - lls.START[1:]) < 0.02
                ks.append(K)
            assert ks == want, (t, a, ks, want)
            per_agent.append(ks)
        out.append(per_agent)
    ora.close()
    return out


def in_long_loop(ks):
    """per step: has an earlier step of this rollout had K > 16 (the wave runs the long loop)?"""
    seen, out = False, []
    for K in ks:
        out.append(seen)
        seen = seen or K > 16
    return out


def every_heuristic(sc, per_agent, pred):
    """pred(ks) holds for at least one agent of each heuristic"""
    return all(any(pred(per_agent[a]) for a in range(sc["n_agents"]) if sc["agent_types"][a] == ty)
               for ty in sorted(set(sc["agent_types"].tolist())))


def _short_long_short_long(ks):
    """short steps, a step with K >= 25, directly behind the long run K <= 3 with K > 0, later K > 16 again"""
    for i, K in enumerate(ks):
        if K >= 25 and i > 0 and all(q <= 16 for q in ks[:i]):
            j = i
            while j < len(ks) and ks[j] > 16:
                j += 1
            return j < len(ks) and 0 < ks[j] <= 3 and any(q > 16 for q in ks[j + 1:])
    return False


@pytest.mark.parametrize("name,moving,sent_near", lls.cases())
def test_scene_holds_its_k_sequences(oracle, scenes, name, moving, sent_near):
    sc = lls.build_scene(scenes, name, moving, sent_near)
    assert sc["obstacles"].shape == (lls.M + 1, 7) and lls.M <= 60 and sc["max_prediction_steps"] <= 64
    assert sc["n_agents"] == 7 and sorted(set(sc["agent_types"].tolist())) == [1, 2, 3, 4, 5, 6] and (sc["agent_types"] == 5).sum() == 2
    assert bool(sc["obstacles"][:-1, 3:6].any()) == bool(moving)
    seqs = k_sequences(oracle, sc, name, moving)
    for t in range(TICKS):      # no rollout stays in the short loop
        assert every_heuristic(sc, seqs[t], lambda ks: any(in_long_loop(ks)))
    if name == "runs":
        # short -> long -> short with a stale second chunk -> long again; an empty shell inside the long loop (the early
        # return); a long step as the last one before the capacity ends the rollout
        for t in (0, 1):
            assert every_heuristic(sc, seqs[t], _short_long_short_long)
        assert every_heuristic(sc, seqs[0], lambda ks: any(K == 0 and lng for K, lng in zip(ks, in_long_loop(ks))))
        assert every_heuristic(sc, seqs[0], lambda ks: ks[-1] > 16 and len(ks) == sc["max_prediction_steps"] - 1)
    else:
        # a long FIRST step, and every chunk boundary met inside the long loop
        assert every_heuristic(sc, seqs[1], lambda ks: ks[0] > 16)
        for t in range(TICKS):
            for want in (16, 17, 32, 33):
                assert every_heuristic(sc, seqs[t], lambda ks: any(K == want and lng for K, lng in zip(ks, in_long_loop(ks)))), (t, want)
