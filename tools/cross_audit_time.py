"""Time of the cross audit (pmaf_cross_audit / pmaf_select_pair) next to the two figures it is to be judged by, per size
N x H (two populations of N agents, scenes.dual_arm_scenes, horizon H):
  pair      HIP events on the handle's stream around one pmaf_select_pair call after the rollout has finished:
            k_cross_audit, the two stages of the pair reduction, 32 bytes back -- the audit WITHOUT the matrix copy;
  matrix    the same around one pmaf_cross_audit call: k_cross_audit and the copy of the [N][N] matrix to the host;
            for both also the host's wall clock around the call (what the caller waits);
  rollout   the same handle's rollout kernel, pmaf_get_kernel_stats (HIP events on its dispatch);
  host      today's alternative: pmaf_get_paths (the copy of all paths of both populations) + the same loop in numpy,
            host wall clock, median of --host-calls calls (it takes seconds at 2 x 1024).
Median of --calls calls after --warmup; every call audits a fresh rollout (one tick in front of it, drained). Every
size runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/cross_audit_time.py [--calls 20] [--warmup 5] [--host-calls 3] [256x200 1024x200 ...]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def host_cross_audit(pa, na, pb, nb, separation, right_assoc):
    """the reference loop in numpy: clearance [Na][Nb]; one row of A against all of B per pass"""
    cap = pa.shape[1]
    k = np.arange(cap)
    ha = np.take_along_axis(pa, np.minimum(k[None, :], np.maximum(na, 1)[:, None] - 1)[:, :, None], axis=1)
    hb = np.take_along_axis(pb, np.minimum(k[None, :], np.maximum(nb, 1)[:, None] - 1)[:, :, None], axis=1)
    out = np.empty((pa.shape[0], pb.shape[0]))
    for i in range(pa.shape[0]):
        d = ha[i][None] - hb
        sq = d * d
        s = sq[..., 0] + (sq[..., 1] + sq[..., 2]) if right_assoc else (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        valid = k[None, :] < np.maximum(na[i], nb)[:, None]
        out[i] = np.sqrt(np.where(valid, s, np.inf).min(axis=1)) - separation
    out[na == 0, :] = np.inf
    out[:, nb == 0] = np.inf
    return out


def measure(size, calls, warmup, host_calls):
    pm = g.load_package()
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    order = pm.load_library().pmaf_eval_order()
    N, H = (int(v) for v in size.split("x"))
    arms = pm.scenes.dual_arm_scenes(N, H, 32)
    sc = arms[0]
    starts = np.stack([s["start"] for s in arms])
    obs = np.stack([s["obstacles"] for s in arms])
    sep = sc.get("radius", 0.05) + 0.1
    h = pm.PmafPlanner(arms, device=0, mgr_init_pos=starts)
    h.set_initial_position(starts)
    h.set_profiling(True)
    stream = C.c_void_p(h.stream())

    def timed(fn):
        assert hip.hipEventRecord(ev[0], stream) == 0
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return r, ms.value * 1e3, (t1 - t0) * 1e6

    pair_us, pair_wall, mat_us, mat_wall, host_us = [], [], [], [], []
    for it in range(warmup + calls):
        if it == warmup:
            h.stop()
            h.reset_kernel_stats()
        h.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
        h.stop()
        sel, us, wall = timed(lambda: h.select_pair(0, 1, sep, 0.05))
        clr, us2, wall2 = timed(lambda: h.cross_audit(0, 1, sep))
        if it >= warmup:
            pair_us.append(us); pair_wall.append(wall); mat_us.append(us2); mat_wall.append(wall2)
        if it >= warmup + calls - host_calls:
            t2 = time.perf_counter()
            paths, n = h.paths()
            ref = host_cross_audit(paths[0], n[0], paths[1], n[1], sep, order)
            host_us.append((time.perf_counter() - t2) * 1e6)
            assert (clr == ref).all(), "the audit and the numpy loop disagree"
            assert sel["clearance"] == clr[sel["pair"]], "the selected pair's clearance is not the matrix entry"
    h.stop()
    ms, launches, _ = h.kernel_stats()
    steps = int(np.maximum(n[0][:, None], n[1][None, :]).sum())
    print("%s: 2 x %d agents, cap %d, %.1f M pair-steps | select_pair (audit + reduction, no matrix copy) %.1f us (events; "
          "caller's wall clock %.1f us) | cross_audit with the matrix copy %.1f us (wall clock %.1f us) | rollout kernel "
          "%.1f us | get_paths + numpy loop %.0f us (median of %d) | median of %d calls" %
          (size, N, h.cap, steps / 1e6, np.median(pair_us), np.median(pair_wall), np.median(mat_us), np.median(mat_wall),
           ms / max(launches, 1) * 1e3, np.median(host_us), host_calls, calls), flush=True)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", default=["256x200", "1024x200"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one size [s]")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        measure(args.sizes[0], args.calls, args.warmup, args.host_calls)
        return
    for size in args.sizes:   # one process and one time limit per size; nothing more is started after a failure
        rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
                              "--calls", str(args.calls), "--warmup", str(args.warmup), "--host-calls", str(args.host_calls), size])
        if rc != 0:
            sys.exit("cross_audit_time: %s ended with status %d; stopping" % (size, rc))


if __name__ == "__main__":
    main()
