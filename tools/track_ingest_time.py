"""What it costs to hand a full set of obstacle tracks to a handle (include/pmaf.h "obstacle tracks" / "obstacle tracks
from device memory"), one row per shape, all in one process on one box. The sides, each the host's wall clock round
the call(s) on an idle handle:
  (a) host call           pmaf_set_obstacle_tracks from a host array [L][M][6] of doubles;
  (b) tensor -> host call what a torch user whose predictor runs on the same GPU does without the device call: device
                          tensor (float64, [L][M][6]) -> .cpu().numpy() -> pmaf_set_obstacle_tracks;
  (c) device call F64/6   pmaf_set_obstacle_tracks_device on that tensor;
  (d) device call F32/3   pmaf_set_obstacle_tracks_device on a float32 tensor of positions only, [L][M][3].
The ingest kernels' own time is not measured here: events recorded from outside the call would bracket its copies and
waits as well and merely repeat the wall clock. It comes from a `rocprofv3 --kernel-trace --stats` run of this script
(k_ftingest_check, k_ftingest_store; profiles/track_ingest.md).
Rows: C2's dynamic scene (64 agents x 200 steps x 32 obstacles) and C1 (16 x 100 x 9). --warmup samples, then the median
of --calls with min .. max, the sides interleaved sample by sample. Prints a markdown table (profiles/track_ingest.md
keeps one run's output).
usage: python tools/track_ingest_time.py [--calls 20] [--warmup 5]"""
import argparse
import os
import sys
import time

import numpy as np
import torch  # before the library: one HIP runtime per process

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def cell(v):
    v = np.asarray(v)
    return "%.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    pm = g.load_package()
    print("| row | side | wall us: median (min .. max) |")
    print("|---|---|---|")
    for label, sc in (("C2 dynamic 64 x 200 x 32", pm.scenes.config_scene("C2", dynamic=True)), ("C1 16 x 100 x 9", pm.scenes.config_scene("C1"))):
        cap = int(sc["max_prediction_steps"])
        M = len(sc["obstacles"]) - 1
        rng = np.random.default_rng(3)
        x = rng.uniform(-0.8, 0.8, (1, M, 3)) + np.cumsum(rng.uniform(-2e-3, 2e-3, (cap, M, 3)), axis=0)
        host6 = np.ascontiguousarray(np.concatenate([x, rng.uniform(-0.5, 0.5, (cap, M, 3))], axis=2))
        t6 = torch.from_numpy(host6).to("cuda:0")
        t3 = torch.from_numpy(np.ascontiguousarray(x.astype(np.float32))).to("cuda:0")
        h = pm.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
        sides = {
            "(a) host call, %d x %d x 6 doubles" % (cap, M): lambda: h.set_obstacle_tracks(host6),
            "(b) tensor -> .cpu().numpy() -> host call": lambda: h.set_obstacle_tracks(t6.cpu().numpy()),
            "(c) device call F64 / 6": lambda: h.set_obstacle_tracks_device(t6),
            "(d) device call F32 / 3": lambda: h.set_obstacle_tracks_device(t3),
        }
        wall = {k: [] for k in sides}
        torch.cuda.synchronize()
        for it in range(args.warmup + args.calls):
            for k, call in sides.items():
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                if it >= args.warmup:
                    wall[k].append((t1 - t0) * 1e6)
        for k in sides:
            print("| %s | %s | %s |" % (label, k, cell(wall[k])))
        a, b, c, d = (np.median(wall[k]) for k in sides)
        print("| %s | (c) / (a), (c) / (b), (d) / (a), (d) / (b) | %.2f, %.2f, %.2f, %.2f |" % (label, c / a, c / b, d / a, d / b))
        sys.stdout.flush()
        h.close()


if __name__ == "__main__":
    main()
