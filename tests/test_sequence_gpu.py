"""Interleaved track, audit and selection calls on the GPU, held to the composed model at tolerance 0: every seeded
sequence of tests/sequence_cases.py runs op by op on a PmafPlanner and on a sequence_model.ModelHandle; after every op the
op's own return value (best indexes, every output of an audit or selection, getter contents, a refusal's code) and,
after every op that can change state, paths, n_points, costs, rot_vecs, known, min_obs_dist, success, agent_vel,
real_state, best, get_repulsive_track and get_obstacle_tracks are compared with assert_array_equal (NaNs equal). The kernels'
own modules hold the arithmetic; this one holds the ORDER rules of include/pmaf.h: which buffer, length and offset a
launch or an audit is handed after a particular sequence of calls. tests/test_sequence_model.py holds the model to the
per-feature references and shows which rule each sequence is sensitive to. The model takes the evaluation order from the
oracle, so the file passes unchanged under PMAF_VARIANT=rassoc."""
import numpy as np
import pytest

import sequence_cases as cases
import sequence_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("PMAF_SUM", "PMAF_FORCE_GENERIC", "PMAF_PLAIN_STEP", "PMAF_MW", "PMAF_W64_SLICE"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_sequence_equals_the_model(pmaf, oracle, scenes, monkeypatch, seed):
    shape, P, ops = cases.sequence(seed)
    ctx = cases.context(oracle, scenes, shape, P)
    for k, v in ctx.env.items():
        monkeypatch.setenv(k, v)

    def device():
        pl = pmaf.PmafPlanner(ctx.scs, device=0, mgr_init_pos=ctx.starts)
        cfg = pl.launch_config()
        assert cfg["lanes_per_agent"] == 64 and cfg["waves_per_agent"] == 1 and not cfg["priority_slices"]
        return pl

    got = cases.trace(seed, ctx, ops, device)
    want = cases.trace(seed, ctx, ops, lambda: model.ModelHandle(oracle, ctx.scs))
    try:
        bad = cases.first_mismatch(seed, got, want)
    finally:
        got.close()
        want.close()
    if bad is not None:
        print(cases.describe(bad))
        print("the sequence:", [(i, op, args) for i, (op, args) in enumerate(ops)][:bad[1] + 1])
        assert bad[4] is not None, cases.describe(bad)
        np.testing.assert_array_equal(np.squeeze(bad[4]), np.squeeze(bad[5]),
                                      err_msg="seed %d op %d (%s) field %s" % bad[:4])
        raise AssertionError(cases.describe(bad))
