"""What the obstacle tracks' device-side source costs (include/pmaf.h "obstacle tracks", pmaf_couple_obstacle_tracks)
against the host's way of getting the SAME tracks into the rollout, in one process on one box, the sides interleaved
sample by sample. Shape: C2's, two arms (P = 2, 64 agents x 200 steps x 32 obstacles), four attached columns per arm
(the other arm's end effector, a carried sphere, two link spheres), shift 1. Both handles run the node's five-call tick
  stop -> evaluate -> [host side only: get_paths + build + set_obstacle_tracks] -> move_real -> reset_agents -> start
and follow bit-identical tracks (asserted: the two handles' paths are equal after every tick):
  device   pmaf_couple_obstacle_tracks once; k_fcouple_take rides on pmaf_reset_agents, k_fcouple_compose on pmaf_start
  host     per tick: pmaf_get_paths (the selected paths come back), the composition in numpy (the unattached columns'
           straight lines are computed once and cached: the list does not change), pmaf_set_obstacle_tracks (transpose
           to [L][6][64] and upload) -- what a caller had to do before the coupling existed
Reported, --warmup ticks, then the median of --calls with min .. max:
  the host way's three parts and their sum (wall clock);
  the wall clock of reset_agents + start + stop on either handle (the same rollout kernel: what differs is the two small
  launches), and the rollout kernel's own time on either (events on its dispatch: pmaf_set_profiling);
  with --trace DIR: the durations of k_fcouple_take and k_fcouple_compose out of a kernel trace of THIS script
  (rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/field_couple_time.py): the library hands out no
  events on those two launches (the ABI gained one export, not a profiling interface), so their device time is read
  from the trace; the last --calls dispatches of each.
Prints a markdown table (profiles/field_couple.md keeps one run's output).
usage: python tools/field_couple_time.py [--calls 20] [--warmup 5] | --trace DIR [--calls 20]"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

SHIFT = 1
# (column, scale, anchor) per arm: end effector, a carried sphere, two spheres along the forearm (base 0.5 m below)
ATTACH = [(0, 1.0, (0.0, 0.0, 0.0)), (1, 1.0, (0.0, 0.0, -0.12)), (2, 0.75, (-0.1125, 0.0, 0.05)), (3, 0.5, (-0.225, 0.0, 0.1))]


def cell(v):
    v = np.asarray(v)
    return "%.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def straight_lines(obstacles, dt, n):
    o = np.asarray(obstacles, dtype=np.float64)[:-1]
    out = np.zeros((n, len(o), 6))
    q = o[:, 0:3].copy()
    for k in range(n):
        out[k, :, 0:3] = q
        out[k, :, 3:6] = o[:, 3:6]
        q = q + o[:, 3:6] * dt
    return out


def compose(lines, path, n, dt, cap):
    """the contract's composition for one arm, vectorised: every rounding a separate numpy operation"""
    out = lines.copy()
    first = min(SHIFT, n - 1)
    y = path[first:n]
    k = np.minimum(np.arange(cap), len(y) - 1)
    for col, s, a in ATTACH:
        x = np.asarray(a)[None, :] + np.float64(s) * y
        u = np.zeros_like(x)
        if len(x) > 1:
            u[:-1] = (x[1:] - x[:-1]) / np.float64(dt)
        out[:, col, 0:3] = x[k]
        out[:, col, 3:6] = u[k]
    return out


def trace(directory, calls):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under " + directory
    dur = {"k_fcouple_take": [], "k_fcouple_compose": [], "k_rollout_w64_ftrack": []}
    for f in files:
        for row in csv.DictReader(open(f)):
            for k in dur:
                if k in row["Kernel_Name"]:
                    dur[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    print("| kernel | dispatches in the trace | device us, the last %d: median (min .. max) |" % calls)
    print("|---|---|---|")
    for k, v in dur.items():
        if v:
            print("| %s | %d | %s |" % (k, len(v), cell(v[-calls:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        return trace(args.trace, args.calls)
    pm = g.load_package()
    arms = pm.scenes.dual_arm_scenes(n_agents=64)
    sc = arms[0]
    P, M, cap, dt = 2, len(sc["obstacles"]) - 1, int(sc["max_prediction_steps"]), sc["dt"]
    starts = np.stack([s["start"] for s in arms])
    live = np.stack([s["obstacles"] for s in arms])
    hs = {}
    for k in ("device", "host"):
        h = pm.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        h.set_initial_position(starts)
        h.set_profiling(True)
        hs[k] = h
    src = np.full((P, M), -1, dtype=np.int32)
    scale, anchor = np.ones((P, M)), np.zeros((P, M, 3))
    for col, s, a in ATTACH:
        src[0, col], src[1, col] = 1, 0
        scale[:, col], anchor[:, col] = s, a
    hs["device"].couple_obstacle_tracks(src, scale, anchor, SHIFT)
    lines = [straight_lines(o, dt, cap) for o in live]
    for h in hs.values():
        h.rollout()
    rows = {k: dict(kern=[], tail=[]) for k in hs}
    host = dict(get=[], build=[], up=[], total=[])
    for it in range(args.warmup + args.calls):
        keep = it >= args.warmup
        for k, h in hs.items():
            h.stop()
            b = h.evaluate(sc["cost_gains"], sc["ws_limits"])
            if k == "host":
                t0 = time.perf_counter()
                paths, n = h.paths()
                t1 = time.perf_counter()
                tracks = [compose(lines[p], paths[1 - p][b[1 - p]], int(n[1 - p][b[1 - p]]), dt, cap) for p in range(P)]
                t2 = time.perf_counter()
                h.set_obstacle_tracks(tracks)
                t3 = time.perf_counter()
                if keep:
                    host["get"].append((t1 - t0) * 1e6); host["build"].append((t2 - t1) * 1e6)
                    host["up"].append((t3 - t2) * 1e6); host["total"].append((t3 - t0) * 1e6)
            h.move_real(live, dt, 1, b)
            pos, vel, _ = h.real_state()
            h.reset_kernel_stats()
            t0 = time.perf_counter()
            h.reset_agents(pos, vel, live)
            h.start()
            h.stop()
            t1 = time.perf_counter()
            ms, launches, _ = h.kernel_stats()
            assert launches == 1
            if keep:
                rows[k]["kern"].append(ms * 1e3); rows[k]["tail"].append((t1 - t0) * 1e6)
        a, c = hs["device"].paths(), hs["host"].paths()
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]), "tick %d: the two handles' paths differ" % it
        ta, tc = hs["device"].get_obstacle_tracks()[0], hs["host"].get_obstacle_tracks()[0]
        assert all(np.array_equal(x, y) for x, y in zip(ta, tc)), "tick %d: the two handles' tracks differ" % it
    label = "C2 shape, 2 x 64 x %d x %d, %d attached columns per arm" % (cap - 1, M, len(ATTACH))
    print("| row | what | us: median (min .. max) |")
    print("|---|---|---|")
    print("| %s | host way: pmaf_get_paths | %s |" % (label, cell(host["get"])))
    print("| %s | host way: composition in numpy | %s |" % (label, cell(host["build"])))
    print("| %s | host way: pmaf_set_obstacle_tracks | %s |" % (label, cell(host["up"])))
    print("| %s | host way: sum, per tick | %s |" % (label, cell(host["total"])))
    for k in hs:
        print("| %s | %s handle: reset_agents + start + stop wall | %s |" % (label, k, cell(rows[k]["tail"])))
        print("| %s | %s handle: rollout kernel (events) | %s |" % (label, k, cell(rows[k]["kern"])))
    d = np.median(rows["device"]["tail"]) - np.median(rows["host"]["tail"])
    print("| %s | device - host handle, reset_agents + start + stop wall (the two small launches) | %.1f |" % (label, d))
    print("| %s | paths and tracks of the two handles bit-identical after every tick | yes (%d ticks) |" % (label, args.warmup + args.calls))
    for h in hs.values():
        h.close()


if __name__ == "__main__":
    main()
