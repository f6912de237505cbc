"""What the clear selection with timing slack costs (include/pmaf.h "clear selection with timing slack"), all in one
process on one box: pmaf_select_clear_slack against pmaf_select_clear_tracked of the same library on one handle of
2 populations x 256 agents x 200 steps x 32 field obstacles (the dynamic synthetic scene), behind one rollout and one
pmaf_evaluate, the field obstacles on tracks of 200 points (the iterated straight lines: the tracked instances of both
kernels run). Rows: horizon 200 and 50; bands (0, 0), (3, 3), (10, 10). HIP events on the handle's stream around each call
(the stream is idle: the rollout is drained and every call waits for its own record), the host's wall clock around the
same call beside them, as tools/tracked_audit_time.py does. The calls differ in the audit kernel alone
(k_obs_slack_audit<true> against k_ft_select_audit). --warmup samples, then the median of --calls with min .. max (the
run-to-run spread), the sides interleaved sample by sample. --untracked drops the tracks (k_obs_slack_audit<false>
against k_select_audit).
Prints a markdown table (profiles/obstacle_slack_audit.md keeps one run's output).
usage: python tools/obstacle_slack_time.py [--calls 20] [--warmup 5] [--untracked]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

P, N, CAP, M = 2, 256, 200, 32
BANDS = ((0, 0), (3, 3), (10, 10))


def straight_lines(obstacles, dt, n):
    """[n][M][6]: the iterated o_i + k v_i dt (multiply, then add) with the constant velocities"""
    o = np.asarray(obstacles, dtype=np.float64)[:-1]
    out = np.zeros((n, len(o), 6))
    q = o[:, 0:3].copy()
    for k in range(n):
        out[k, :, 0:3] = q
        out[k, :, 3:6] = o[:, 3:6]
        q = q + o[:, 3:6] * dt
    return out


def cell(v):
    v = np.asarray(v)
    return "%.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--untracked", action="store_true")
    args = ap.parse_args()
    pm = g.load_package()
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed(stream, fn):
        """(result, device us between two events around fn on the stream, host wall clock us of fn)"""
        assert hip.hipEventRecord(ev[0], stream) == 0
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return out, ms.value * 1e3, (t1 - t0) * 1e6

    scs = [pm.scenes.synthetic_scene(N, CAP - 1, M, config_id=2, scene_id=p, dynamic=True) for p in range(P)]
    starts = np.stack([s["start"] for s in scs])
    h = pm.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    try:
        h.set_initial_position(starts)
        h.rollout()
        h.evaluate(scs[0]["cost_gains"], scs[0]["ws_limits"])
        n = np.asarray(h.n_points())
        live = np.stack([pm.scenes.advance_live_obstacles(s["obstacles"]) for s in scs])
        if not args.untracked:
            h.set_obstacle_tracks([straight_lines(live[p], scs[p]["dt"], CAP) for p in range(P)])
        stream = C.c_void_p(h.stream())
        print("%d x %d agents, path lengths %d .. %d (median %d) of %d, %d field obstacles, %s" % (
            P, N, n.min(), n.max(), np.median(n), CAP, M, "no tracks" if args.untracked else "tracks of %d points" % CAP))
        print()
        print("| horizon | call | band (late, early) | device us: median (min .. max) | / tracked | wall us: median (min .. max) | n_clear |")
        print("|---|---|---|---|---|---|---|")
        for horizon in (200, 50):
            sides = [("pmaf_select_clear_tracked", None)] + [("pmaf_select_clear_slack", b) for b in BANDS]
            dev = {s: [] for s in sides}
            wall = {s: [] for s in sides}
            last = {}
            for it in range(args.warmup + args.calls):
                for s in sides:
                    if s[1] is None:
                        fn = lambda: h.select_clear_tracked(live, 0.05, horizon, prev=[1] * P)
                    else:
                        fn = lambda: h.select_clear_slack(live, 0.05, horizon, s[1][0], s[1][1], prev=[1] * P)
                    last[s], d_us, w_us = timed(stream, fn)
                    if it >= args.warmup:
                        dev[s].append(d_us)
                        wall[s].append(w_us)
            base = np.median(dev[sides[0]])
            for s in sides:
                print("| %d | %s | %s | %s | %.2f | %s | %s |" % (horizon, s[0], "-" if s[1] is None else "(%d, %d)" % s[1], cell(dev[s]),
                                                                np.median(dev[s]) / base, cell(wall[s]),
                                                                np.asarray(last[s]["n_clear"]).tolist()))
            same = all(np.array_equal(np.asarray(last[sides[0]][k]), np.asarray(last[sides[1]][k])) for k in last[sides[0]])
            print("| %d | (0, 0) equals the tracked call bit for bit: %s | | | | | |" % (horizon, same))
            sys.stdout.flush()
    finally:
        h.close()


if __name__ == "__main__":
    main()
