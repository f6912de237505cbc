"""Time of the cross audit with timing slack (pmaf_cross_audit_slack / pmaf_select_pair_slack) next to the figures it is
to be judged by, per case NxH:LATE_A,LATE_B (two populations of N agents, scenes.dual_arm_scenes, horizon H):
  slack pair   HIP events on the handle's stream around one pmaf_select_pair_slack call after the rollout has finished:
               k_cross_audit_slack, the two stages of the pair reduction, the result and the pair's two steps back --
               the audit WITHOUT the matrix copy; and the time per million admitted pair-steps;
  slack matrix the same around one pmaf_cross_audit_slack call (clearance only): the kernel and the [N][N] copy;
  pair         the same run's pmaf_select_pair (k_cross_audit: the slack (0, 0) through the un-slacked kernel), with its
               time per million pair-steps;
  rollout      the same handle's rollout kernel, pmaf_get_kernel_stats (HIP events on its dispatch);
  host         the caller's alternative: pmaf_get_paths + the same banded loop in numpy, host wall clock, median of
               --host-calls calls (seconds at the larger cases), compared bit for bit with the call's matrix.
Median of --calls calls after --warmup; every call audits a fresh rollout (one tick in front of it, drained). Every
case runs in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/slack_audit_time.py [--calls 20] [--warmup 5] [--host-calls 1] [256x200:0,0 256x200:5,5 ...]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def host_slack_audit(pa, na, pb, nb, separation, late_a, late_b, right_assoc):
    """the reference loop in numpy: clearance [Na][Nb]; one row of A and one offset l - k per pass"""
    cap = pa.shape[1]
    k = np.arange(cap)
    ha = np.take_along_axis(pa, np.minimum(k[None, :], np.maximum(na, 1)[:, None] - 1)[:, :, None], axis=1)
    hb = np.take_along_axis(pb, np.minimum(k[None, :], np.maximum(nb, 1)[:, None] - 1)[:, :, None], axis=1)
    out = np.empty((pa.shape[0], pb.shape[0]))
    for i in range(pa.shape[0]):
        big_k = np.maximum(na[i], nb)[:, None]
        best = np.full(pb.shape[0], np.inf)
        for s in range(-min(late_b, cap - 1), min(late_a, cap - 1) + 1):
            ka = k[max(0, -s):cap - max(0, s)]
            d = ha[i][ka][None] - hb[:, ka + s]
            sq = d * d
            d2 = sq[..., 0] + (sq[..., 1] + sq[..., 2]) if right_assoc else (sq[..., 0] + sq[..., 1]) + sq[..., 2]
            valid = (ka[None, :] < big_k) & (ka[None, :] + s < big_k)
            best = np.minimum(best, np.where(valid, d2, np.inf).min(axis=1))
        out[i] = np.sqrt(best) - separation
    out[na == 0, :] = np.inf
    out[:, nb == 0] = np.inf
    return out


def admitted_pair_steps(na, nb, late_a, late_b):
    big_k = np.maximum(na[:, None], nb[None, :])
    total = 0
    for kk, count in zip(*np.unique(big_k, return_counts=True)):
        k = np.arange(int(kk))
        total += int(count) * int((np.minimum(kk - 1, k + late_a) - np.maximum(0, k - late_b) + 1).sum())
    return total, int(big_k.sum())


def measure(case, calls, warmup, host_calls):
    pm = g.load_package()
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    order = pm.load_library().pmaf_eval_order()
    size, late = case.split(":")
    N, H = (int(v) for v in size.split("x"))
    late_a, late_b = (int(v) for v in late.split(","))
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

    t = {k: [] for k in ("slack_pair", "slack_pair_wall", "slack_mat", "slack_mat_wall", "pair", "host")}
    for it in range(warmup + calls):
        if it == warmup:
            h.stop()
            h.reset_kernel_stats()
        h.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
        h.stop()
        sel, us, wall = timed(lambda: h.select_pair_slack(0, 1, sep, 0.05, late_a, late_b))
        clr, us2, wall2 = timed(lambda: h.cross_audit_slack(0, 1, sep, late_a, late_b))
        _, us3, _ = timed(lambda: h.select_pair(0, 1, sep, 0.05))
        if it >= warmup:
            t["slack_pair"].append(us); t["slack_pair_wall"].append(wall); t["slack_mat"].append(us2)
            t["slack_mat_wall"].append(wall2); t["pair"].append(us3)
        if it >= warmup + calls - host_calls:
            t2 = time.perf_counter()
            paths, n = h.paths()
            ref = host_slack_audit(paths[0], n[0], paths[1], n[1], sep, late_a, late_b, order)
            t["host"].append((time.perf_counter() - t2) * 1e6)
            assert (clr == ref).all(), "the audit and the numpy loop disagree"
            assert sel["clearance"] == clr[sel["pair"]], "the selected pair's clearance is not the matrix entry"
    h.stop()
    ms, launches, _ = h.kernel_stats()
    steps, plain_steps = admitted_pair_steps(n[0], n[1], late_a, late_b)
    m = {k: float(np.median(v)) for k, v in t.items()}
    print("%s: 2 x %d agents, cap %d, slack (%d, %d), %.1f M admitted pair-steps | select_pair_slack (audit + reduction, no "
          "matrix copy) %.1f us (events; caller's wall clock %.1f us) = %.3f us per M pair-steps | cross_audit_slack with the "
          "matrix copy %.1f us (wall clock %.1f us) | select_pair %.1f us = %.3f us per M of its %.1f M pair-steps | rollout "
          "kernel %.1f us | get_paths + numpy loop %.0f us (median of %d) | median of %d calls" %
          (case, N, h.cap, late_a, late_b, steps / 1e6, m["slack_pair"], m["slack_pair_wall"], m["slack_pair"] / (steps / 1e6),
           m["slack_mat"], m["slack_mat_wall"], m["pair"], m["pair"] / (plain_steps / 1e6), plain_steps / 1e6,
           ms / max(launches, 1) * 1e3, m["host"], host_calls, calls), flush=True)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["256x200:0,0", "256x200:5,5", "256x200:30,30", "1024x200:5,5"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one case [s]")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        measure(args.cases[0], args.calls, args.warmup, args.host_calls)
        return
    for case in args.cases:   # one process and one time limit per case; nothing more is started after a failure
        rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child",
                              "--calls", str(args.calls), "--warmup", str(args.warmup), "--host-calls", str(args.host_calls), case])
        if rc != 0:
            sys.exit("slack_audit_time: %s ended with status %d; stopping" % (case, rc))


if __name__ == "__main__":
    main()
