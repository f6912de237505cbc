"""k_manager's selection (csrc/pmaf_k_misc.hip: cost assembly, first minimum over the population, 0.9 hysteresis, the
winner's type and random vectors into the real agent's step) against the independent high-precision reference at every
shape: the designed selections of tests/hp_select.py -- exact ties, the only minimum and the stored best agent placed
by agent index -- at the smallest sizes at which each path of the four-agents-per-lane assembly exists (slots 1-3,
second and third pass, clamped padding loads, the cross-lane index rule, LDS reads at 64 and above, odd N, more than
one population). tests/test_hp_select.py shows on the CPU that every case is decidable by the reference alone and
that planners selecting by a plausible wrong rule fail on them.

The cost gains (hp_select.COST_GAINS) keep all four per-agent result streams in every compared cost: cost_ws, goal_dist,
path_len and, through a non-zero safe-distance gain, min_obs.

Costs are held to the reference's bound; indices, types and flags exactly; nothing may be undecidable, and the count of
compared selections is asserted. Run with -s to see the per-case report.
"""
import numpy as np
import pytest

import hp_reference as hp
import hp_select as hs
import hp_shadow as sh

pytestmark = pytest.mark.gpu

POLICY_KW = {"xact": {}, "fma": {"contracted": True}}


def _make(pmaf, policy="xact", lpa=0, expect=None):
    def make(sc):
        scs = [sc] if isinstance(sc, dict) else sc
        starts = np.stack([s["start"] for s in scs])
        pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=starts[0] if len(scs) == 1 else starts, lanes_per_agent=lpa,
                              **POLICY_KW[policy])
        cfg = pl.launch_config()
        for k, v in (expect or {}).items():
            assert cfg[k] == v, (k, cfg)
        return pl
    return make


def _case(pmaf, scenes, N, kind, where=None, entry="tick", policy="xact", lpa=0, expect=None, key="default",
          inspect=None, seed=hs.SEED):
    A = hp.Arith(policy)
    st = sh.Stats("%s [%s, %s]" % (hs.case_id(N, kind, where, entry), policy, key))
    rs = sh.Stats("rollouts")
    hs.designed_case(_make(pmaf, policy, lpa, expect), scenes, N, seed, kind, A, st, "%s/%s" % (policy, key),
                     where=where, entry=entry, rollout_stats=rs, inspect=inspect)
    hs.assert_decided(st, rs, N)


@pytest.mark.parametrize("N,kind", hs.TIE_CASES, ids=[hs.case_id(*c) for c in hs.TIE_CASES])
def test_tie_layouts(pmaf, scenes, N, kind):
    """has_best = 0: the first minimum of the population, with the winner's exact copies in the same lane's next slot,
    the next pass, at N - 1, in a lower lane at a higher index, everywhere, or the only minimum in the padded tail"""
    _case(pmaf, scenes, N, kind)


@pytest.mark.parametrize("N,kind,where", hs.PRIOR_CASES, ids=[hs.case_id(*c) for c in hs.PRIOR_CASES])
def test_hysteresis(pmaf, scenes, N, kind, where):
    """the stored best agent (set_best) at an index in 64-255, at 256 or above, or at N - 1: kept when it ties with the
    argmin or costs a little more, left when it costs far more (switch_far: with the argmin itself at 70, so that both
    s_cost[] reads of the hysteresis are at 64 or above); all costs exactly 0 (0 < 0.9 * 0 is false)"""
    _case(pmaf, scenes, N, kind, where)


@pytest.mark.parametrize("N,kind,seed", hs.RECORD_CASES)
def test_winner_type_and_random_vectors_from_a_high_index(pmaf, scenes, N, kind, seed):
    """the selected agent (at N - 1, or at 70 with a copy at 130) is a Random agent and agent 0 is not; the real agent
    latches rotation vectors in the compared step, which a Random agent's heuristic computes from the random vectors
    copied into best_rnd (tests/test_hp_select.py shows the condition and that taking either from index 0 fails)"""
    _case(pmaf, scenes, N, kind, seed=seed)


def _winner_record(pmaf):
    """after the stand-alone evaluate: the record pmaf_write_winner_records packs holds, bit for bit, the cost, index,
    path length and type of the agent the reference selected, and the path that was scored"""
    torch = pytest.importorskip("torch")      # only to own the device buffer

    def inspect(pl, sc, best):
        rec = pl.winner_record_doubles()
        buf = torch.zeros((1, rec), dtype=torch.float64, device="cuda:0")
        pl.write_winner_records(buf.data_ptr(), buf.numel() * 8)
        pl.stop()
        out = pmaf.shard.unpack_winner_records(buf.cpu().numpy(), sc["max_prediction_steps"])[0]
        paths, n = pl.paths()
        assert out["index"] == best and out["n_points"] == n[best] and out["type"] == sh.agent_types(sc)[best], out
        assert out["cost"] == pl.costs()[best]
        np.testing.assert_array_equal(out["path"], paths[best, :n[best]])
    return inspect


@pytest.mark.parametrize("N,kind,where", hs.EVALUATE_CASES, ids=[hs.case_id(*c, entry="evaluate") for c in hs.EVALUATE_CASES])
def test_stand_alone_evaluate_and_winner_record(pmaf, scenes, N, kind, where):
    """pmaf_evaluate (a manager launch that only selects), then move_real with the returned index; the winner record"""
    _case(pmaf, scenes, N, kind, where, entry="evaluate", inspect=_winner_record(pmaf))


# the rollout kernels' post-loop pass writes the cost terms the manager assembles (cost_ws, path_len, goal_dist; min_obs
# comes out of the loop itself), and it differs per kernel family
PRODUCERS = {
    "grp16": dict(lpa=16, expect=dict(lanes_per_agent=16)),
    # (launch_config() has no key that tells the generic kernel from k_rollout_w64 at 64 lanes per agent: the assertion
    # only shows that the mapping was not changed; tests/test_hp_reference_gpu.py::test_generic forces it the same way)
    "generic": dict(lpa=64, expect=dict(lanes_per_agent=64)),
    "fma": dict(policy="fma"),
}
PRODUCER_LAYOUTS = {65: [("tail", None), ("next_slot", None), ("keep_dup", "last")],
                    321: [("tail", None), ("lane_order", None), ("switch", "high")]}


@pytest.mark.parametrize("N", [65, 321])
@pytest.mark.parametrize("producer", list(PRODUCERS))
def test_cost_term_producers(pmaf, scenes, monkeypatch, producer, N):
    if producer == "generic":
        monkeypatch.setenv("PMAF_FORCE_GENERIC", "1")
    for kind, where in PRODUCER_LAYOUTS[N]:
        _case(pmaf, scenes, N, kind, where, key=producer, **PRODUCERS[producer])


@pytest.mark.parametrize("N", [65, 321])
def test_three_populations(pmaf, scenes, N):
    """one handle, P = 3: different fields, gains and goals; the reference's winners are three distinct indices
    (tests/test_hp_select.py), so the pop * N offsets of the results, the costs, the gains and the random vectors are
    all exercised"""
    A = hp.Arith("xact")
    st, rs = sh.Stats("P = 3, N = %d" % N), sh.Stats("rollouts")
    scs = hs.population_scenes(scenes, N)
    pl = _make(pmaf)(scs)
    try:
        best = hs.run_populations(pl, scs, A, st, rollout_stats=rs)
    finally:
        pl.close()
    hs.assert_decided(st, rs, N, 3)
    assert len(set(best)) == 3, best
