"""The K-varying scenes (tests/long_loop_scenes.py, tests/sum_chunk_scenes.py) on EVERY one-slot wave-per-agent rollout
instantiation, not only the four that a default handle launches: the rows of tests/variant_matrix.py. The ordered force
sum of these kernels is one text (csrc/pmaf_rollout_w64_step.hpp, circ_and_scale_w64) compiled per arithmetic policy,
step variant and sum, with hand-placed wait states round its DPP accumulates; a stale second chunk, a missed 17th term or
a wrong wait state in one unit is a fault of that unit's object alone.

Bit-exact legs (tolerance 0 against the CPU oracle, the references and run_and_compare of tests/test_long_loop_gpu.py and
tests/test_sum_chunks_gpu.py): the IEEE policy, the forced general step and the LDS sum compute the reference's bits by
contract -- 7 strict rows x (7 long-loop cases + 10 K x 2 flag pairs), 3 track and 3 ftrack rows x (2 long-loop scenes +
K = 17, 33), and the general step reached through the inputs (mass 2.5; k_attr = 0 for two agents on top) on 4 rows x
K = 17, 33 x 2 flag pairs x 2 variants.

Bounded legs (fast and contracted policies, 8 rows, and the contracted sliced kernel at 1.5 waves per SIMD): tick 0 of
each case shadowed by the high-precision reference under the policy's bound (tests/hp_shadow.py, BOUND_FACTOR 1), at most
K_STEP_MAX_UNDECIDABLE undecidable samples and all seven rollouts compared. tests/test_variant_matrix.py shows on the CPU
that every such case is decidable by the reference alone, and that a dropped 17th term or a stale term fails under this
bound. Which cases: variant_matrix.BOUNDED_LONG_LOOP's docstring -- the scenes whose repulsive obstacle is far away keep
the agents exactly at vel_max on the x axis, which no bound of a policy with rounded roots can decide.

Which body a handle ran is not reported by the device (launch_config() has no policy, step or sum): the rows' routes are
checked in tests/test_variant_matrix.py; here the mapping, the wave count and priority_slices are asserted."""
import pytest
import torch

import long_loop_scenes as lls
import sum_chunk_scenes as scs
import test_hp_reference_gpu as thr
import test_long_loop_gpu as tll
import test_sum_chunks_gpu as tsc
import variant_matrix as vm

pytestmark = pytest.mark.gpu

_ids = dict(ids=lambda r: r.name)


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


@pytest.fixture
def env(monkeypatch):
    return lambda row: vm.apply_env(monkeypatch, row)


# ---- bit-exact legs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,moving,sent_near", lls.cases())
@pytest.mark.parametrize("row", vm.STRICT, **_ids)
def test_strict_row_k_varies(pmaf, oracle, scenes, env, row, name, moving, sent_near):
    sc, ticks, costs = tll.reference(oracle, scenes, name, moving, sent_near)
    env(row)
    tll.run_and_compare(pmaf, sc, ticks, costs, planner_kw=row.kw, tag="%s %s moving=%s sent=%s" % (row.name, name, moving, sent_near))


@pytest.mark.parametrize("moving,sent_near", vm.SUM_CHUNK_STRICT_FLAGS)
@pytest.mark.parametrize("K", scs.KS)
@pytest.mark.parametrize("row", vm.STRICT, **_ids)
def test_strict_row_k_terms(pmaf, oracle, scenes, env, row, K, moving, sent_near):
    sc, ticks, costs = tsc.reference(oracle, scenes, K, moving, sent_near)
    env(row)
    tsc.run_and_compare(pmaf, sc, ticks, costs, planner_kw=row.kw, tag="%s K%d moving=%s sent=%s" % (row.name, K, moving, sent_near))


@pytest.mark.parametrize("variant", vm.GENERAL_VARIANTS)
@pytest.mark.parametrize("moving,sent_near", vm.SUM_CHUNK_STRICT_FLAGS)
@pytest.mark.parametrize("K", vm.GENERAL_KS)
@pytest.mark.parametrize("row", vm.GENERAL_BY_INPUT, **_ids)
def test_general_step_by_input(pmaf, oracle, scenes, env, row, K, moving, sent_near, variant):
    """nothing forced: agent_mass = 2.5 (and k_attr = 0 for agents 1 and 4) is what takes the handle to the general step;
    its own oracle reference (tests/test_sum_chunks.py: K is still held)"""
    sc, ticks, costs = tsc.reference(oracle, scenes, K, moving, sent_near, edit=(variant, lambda s: vm.general_scene(s, variant)))
    assert not vm.plain_input(row, sc)
    env(row)
    tsc.run_and_compare(pmaf, sc, ticks, costs, planner_kw=row.kw, tag="%s K%d %s" % (row.name, K, variant))


@pytest.mark.parametrize("name", sorted(lls.SCENES))
@pytest.mark.parametrize("row", vm.TRACK, **_ids)
def test_track_row_k_varies(pmaf, oracle, scenes, env, row, name):
    track = tll._track(lls.build_scene(scenes, name, False, True))
    sc, ticks, costs = tll.reference(oracle, scenes, name, False, True, track=track)
    env(row)
    tll.run_and_compare(pmaf, sc, ticks, costs, setup=lambda pl: pl.set_repulsive_track(track), planner_kw=row.kw,
                        tag="%s %s" % (row.name, name))


@pytest.mark.parametrize("K", vm.TRACK_KS)
@pytest.mark.parametrize("row", vm.TRACK, **_ids)
def test_track_row_k_terms(pmaf, oracle, scenes, env, row, K):
    track = tsc._track()
    sc, ticks, costs = tsc.reference(oracle, scenes, K, False, True, track=track)
    env(row)
    tsc.run_and_compare(pmaf, sc, ticks, costs, setup=lambda pl: pl.set_repulsive_track(track), planner_kw=row.kw,
                        tag="%s K%d" % (row.name, K))


@pytest.mark.parametrize("name", sorted(lls.SCENES))
@pytest.mark.parametrize("row", vm.FTRACK, **_ids)
def test_ftrack_row_k_varies(pmaf, oracle, scenes, env, row, name):
    ft = tll._obstacle_tracks(lls.build_scene(scenes, name, False, False))
    sc, ticks, costs = tll.reference(oracle, scenes, name, False, False, ftracks=ft)
    env(row)
    tll.run_and_compare(pmaf, sc, ticks, costs, setup=lambda pl: pl.set_obstacle_tracks(ft), planner_kw=row.kw,
                        tag="%s %s" % (row.name, name))


@pytest.mark.parametrize("K", vm.TRACK_KS)
@pytest.mark.parametrize("row", vm.FTRACK, **_ids)
def test_ftrack_row_k_terms(pmaf, oracle, scenes, env, row, K):
    ft = tsc._obstacle_tracks(scs.build_scene(scenes, K, False, False))
    sc, ticks, costs = tsc.reference(oracle, scenes, K, False, False, ftracks=ft)
    env(row)
    tsc.run_and_compare(pmaf, sc, ticks, costs, setup=lambda pl: pl.set_obstacle_tracks(ft), planner_kw=row.kw,
                        tag="%s K%d" % (row.name, K))


# ---- bounded legs -------------------------------------------------------------------------------------------------------
def _shadow(pmaf, row, sc, mod, tag, agents=None, lpa=0):
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=mod.INIT, lanes_per_agent=lpa, **row.kw)
    try:
        cfg = pl.launch_config()
        assert cfg["lanes_per_agent"] == 64 and cfg["waves_per_agent"] == 1, cfg
        assert bool(cfg["priority_slices"]) == row.crowded, cfg
        st = vm.shadow_first_tick(pl, sc, mod.INIT, mod.START, row.policy, "%s %s" % (row.name, tag), agents=agents)
    finally:
        pl.close()
    print("rollout samples compared: %d" % st.rollouts_compared)
    st.assert_ok(thr.K_STEP_MAX_UNDECIDABLE)
    assert st.rollouts_compared >= vm.MIN_ROLLOUT_SAMPLES, st.report()


@pytest.mark.parametrize("name,moving,sent_near", vm.BOUNDED_LONG_LOOP)
@pytest.mark.parametrize("row", vm.BOUNDED, **_ids)
def test_bounded_row_k_varies(pmaf, scenes, env, row, name, moving, sent_near):
    env(row)
    sc = lls.build_scene(scenes, name, moving, sent_near)
    _shadow(pmaf, row, sc, lls, sc["name"])


@pytest.mark.parametrize("K,moving,sent_near", vm.BOUNDED_SUM_CHUNK)
@pytest.mark.parametrize("row", vm.BOUNDED, **_ids)
def test_bounded_row_k_terms(pmaf, scenes, env, row, K, moving, sent_near):
    env(row)
    sc = scs.build_scene(scenes, K, moving, sent_near)
    _shadow(pmaf, row, sc, scs, sc["name"])


@pytest.mark.parametrize("name,moving,sent_near", vm.SLICED_LONG_LOOP)
@pytest.mark.parametrize("row", vm.SLICED, **_ids)
def test_sliced_row_k_varies(pmaf, scenes, env, row, name, moving, sent_near):
    """one population of 1.5 x SIMDs agents (the seven types repeated), agents 0 ... 6 shadowed"""
    env(row)
    simds = torch.cuda.get_device_properties(0).multi_processor_count * 4
    sc = lls.build_scene(scenes, name, moving, sent_near, n_agents=vm.crowded_agents(simds))
    _shadow(pmaf, row, sc, lls, "%s x %d" % (sc["name"], sc["n_agents"]), agents=range(7), lpa=64)
