"""Interleaved track / audit / selection call sequences, device against the composed CPU model, for seeds beyond the
committed ones: the loop of tests/test_sequence_gpu.py (tests/sequence_cases.py, tests/sequence_model.py) over
first_seed ... first_seed + n - 1. Every mismatch is printed as seed / op index / op / field with both values; the exit
status is non-zero if there was one. Anything other than a value mismatch (a device error, an exception of the model)
ends the run at once. Campaign tooling in the way of tools/fuzz_api.py: not called from a test.
usage: python tools/fuzz_sequences.py [n] [first_seed]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

pm = g.load_package()
from oracle import orc  # noqa: E402

import sequence_cases as cases  # noqa: E402
import sequence_model as model  # noqa: E402

orc.build()
orc.set_exp_mode(1)
assert pm.load_library().pmaf_eval_order() == orc.eval_order(), "library and oracle were built with different dot-product associations"
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
first_seed = int(sys.argv[2]) if len(sys.argv) > 2 else len(cases.SEEDS)
bad = 0
t_all = time.time()
for seed in range(first_seed, first_seed + n):
    shape, P, ops = cases.sequence(seed)
    ctx = cases.context(orc, pm.scenes, shape, P)
    for k in ("PMAF_SUM",):
        os.environ.pop(k, None)
    os.environ.update(ctx.env)
    t0 = time.time()
    got = cases.trace(seed, ctx, ops, lambda: pm.PmafPlanner(ctx.scs, device=0, mgr_init_pos=ctx.starts))
    want = cases.trace(seed, ctx, ops, lambda: model.ModelHandle(orc, ctx.scs))
    try:
        miss = cases.first_mismatch(seed, got, want)
    finally:
        got.close()
        want.close()
    print("seed %d %s P %d: %d ops, %.2f s, %s" % (seed, shape, P, len(ops), time.time() - t0, "MISMATCH" if miss else "ok"), flush=True)
    if miss:
        bad += 1
        print(cases.describe(miss), flush=True)
        print("ops up to there:", [(i, o, a) for i, (o, a) in enumerate(ops)][:miss[1] + 1], flush=True)
print("seeds %d mismatches %d in %.0f s" % (n, bad, time.time() - t_all))
sys.exit(1 if bad else 0)
