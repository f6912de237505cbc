"""What the obstacle tracks cost (include/pmaf.h "obstacle tracks"), one row per shape, all in one process on one box:
  rollout    the rollout kernel's own time (events on its dispatch: pmaf_set_profiling) of the same rollout -- the
             population reset to the scene's start in front of every sample -- on two handles of the same scene:
             `untracked` (k_rollout_w64) and `straight lines` (k_rollout_w64_ftrack following the iterated straight
             lines with the constant velocities: the same bits and the same paths, so the comparison is like for
             like; the tracked loop carries six loads and six 64-bit selects more per step and never the bodies that
             assume obstacles at rest);
  upload     the host's wall clock around pmaf_set_obstacle_tracks with a full track set of the shape (cap points) and
             around pmaf_set_obstacle_track_offset (P integers), on an idle handle.
Rows: C2's dynamic scene (64 agents x 200 steps x 32 obstacles) and C1 (16 x 100 x 9; its obstacles rest, so the
untracked side runs the at-rest bodies). --warmup samples, then the median of --calls with min .. max (the run-to-run
spread), the sides interleaved sample by sample. Prints a markdown table (profiles/field_track.md keeps one run's output).
usage: python tools/field_track_time.py [--calls 20] [--warmup 5]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


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
    args = ap.parse_args()
    pm = g.load_package()
    print("| row | side | rollout kernel us: median (min .. max) | agent-steps per launch |")
    print("|---|---|---|---|")
    uploads = []
    for label, sc in (("C2 dynamic 64 x 200 x 32", pm.scenes.config_scene("C2", dynamic=True)), ("C1 16 x 100 x 9", pm.scenes.config_scene("C1"))):
        cap = int(sc["max_prediction_steps"])
        lines = straight_lines(sc["obstacles"], sc["dt"], cap)
        hs = {}
        for k in ("untracked", "straight lines"):
            h = pm.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
            h.set_profiling(True)
            hs[k] = h
        hs["straight lines"].set_obstacle_tracks(lines)
        rows = {k: dict(kern=[], steps=[]) for k in hs}
        paths = {}
        for it in range(args.warmup + args.calls):
            for k, h in hs.items():
                h.set_initial_position(sc["start"])
                h.reset_kernel_stats()
                h.rollout()
                h.stop()
                ms, launches, steps = h.kernel_stats()
                assert launches == 1
                if it >= args.warmup:
                    rows[k]["kern"].append(ms * 1e3)
                    rows[k]["steps"].append(steps)
        for k, h in hs.items():
            paths[k] = h.paths()
            print("| %s | %s | %s | %d |" % (label, k, cell(rows[k]["kern"]), np.median(rows[k]["steps"])))
        same = np.array_equal(paths["untracked"][0], paths["straight lines"][0]) and np.array_equal(paths["untracked"][1], paths["straight lines"][1])
        a, b = np.median(rows["untracked"]["kern"]), np.median(rows["straight lines"]["kern"])
        print("| %s | straight lines / untracked rollout kernel | %.4f (paths bit-identical: %s) | |" % (label, b / a, same))
        # upload: a full track set, and the offset alone
        h = hs["straight lines"]
        full, off = [], []
        for it in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            h.set_obstacle_tracks(lines)
            t1 = time.perf_counter()
            h.set_obstacle_track_offset(it % 7)
            t2 = time.perf_counter()
            if it >= args.warmup:
                full.append((t1 - t0) * 1e6)
                off.append((t2 - t1) * 1e6)
        uploads.append((label, lines.shape, lines.nbytes, full, off))
        sys.stdout.flush()
        for h in hs.values():
            h.close()
    print()
    print("| row | tracks | pmaf_set_obstacle_tracks wall us (binding included) | pmaf_set_obstacle_track_offset wall us |")
    print("|---|---|---|---|")
    for label, shape, nbytes, full, off in uploads:
        print("| %s | %s doubles, %.0f KB | %s | %s |" % (label, "x".join(str(s) for s in shape), nbytes / 1024.0, cell(full), cell(off)))


if __name__ == "__main__":
    main()
