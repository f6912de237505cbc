"""What the repulsive track costs (include/pmaf.h "repulsive track"), one row per shape, all in one process on one box:
  rollout    the rollout kernel's own time (events on its dispatch: pmaf_set_profiling) on two handles of the same scenes
             driven through the same ticks -- `untracked`: the other arm as the sphere at its last set-point, in range
             (today's loop with code for the obstacle), `coupled`: the same handle coupled with shift 1
             (k_rollout_w64_track: one 24-byte wave-uniform load and three selects more per step);
  tick       the host's wall clock around pmaf_tick (returns at the set-point) and around pmaf_tick + pmaf_stop, on ONE
             handle whose coupling is switched on and off from sample to sample: the coupled tick's third launch
             (k_track_from_best between the manager kernel and the rollout).
Rows: C4 (2 x 256 agents x 200 steps x 32 obstacles) and two arms at the shipped task's shape (10 agents x 1 500 steps x
9 obstacles), where the track is longest. 2 x 1 024 agents run the priority-slicing loop, which has no tracked variant.
--warmup ticks, then the median of --calls with min .. max (the run-to-run spread), the sides interleaved sample by
sample. Prints a markdown table (profiles/sentinel_track.md keeps one run's output).
usage: python tools/sentinel_track_time.py [--calls 20] [--warmup 5]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def task_arms(pm):
    arms = []
    for arm, (y0, y1) in enumerate(((-0.12, 0.10), (0.12, -0.10))):
        s = pm.scenes.static1_scene(n_agents=10, horizon=1500, seed=0xC0FFEE00 + 1 * 256 + arm)
        s["start"] = s["start"] + np.array([0.0, y0, 0.0])
        s["goal"] = s["goal"] + np.array([0.0, y1, 0.0])
        arms.append(s)
    return arms


def cell(v):
    v = np.asarray(v)
    return "%.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    pm = g.load_package()
    print("| row | side | rollout kernel us: median (min .. max) | tick wall us | tick + stop wall us |")
    print("|---|---|---|---|---|")
    for label, arms in (("C4 2 x 256 x 200 x 32", pm.scenes.dual_arm_scenes()), ("task shape 2 x 10 x 1500 x 9", task_arms(pm))):
        sc = arms[0]
        starts = np.stack([s["start"] for s in arms])
        hs, cpl = {}, {}
        for k in ("untracked", "coupled", "switched"):
            h = pm.PmafPlanner(arms, device=0, mgr_init_pos=starts)
            h.set_initial_position(starts)
            h.set_profiling(True)
            hs[k] = h
            cpl[k] = pm.shard.DualArmCoupling(np.stack([s["obstacles"] for s in arms]), 0.1)
        hs["coupled"].couple_tracks([1, 0], 1)
        for h in hs.values():
            h.rollout()
        rows = {k: dict(kern=[], tick=[], full=[], steps=[]) for k in ("untracked", "coupled", "switched: uncoupled", "switched: coupled")}

        def sample(key, h, c, keep):
            obs = c.coupled_obstacles(h.real_state()[0])
            h.reset_kernel_stats()
            t0 = time.perf_counter()
            h.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
            t1 = time.perf_counter()
            h.stop()
            t2 = time.perf_counter()
            ms, launches, steps = h.kernel_stats()
            assert launches == 1
            if keep:
                r = rows[key]
                r["kern"].append(ms * 1e3); r["tick"].append((t1 - t0) * 1e6); r["full"].append((t2 - t0) * 1e6); r["steps"].append(steps)

        for it in range(args.warmup + args.calls):
            keep = it >= args.warmup
            sample("untracked", hs["untracked"], cpl["untracked"], keep)
            sample("coupled", hs["coupled"], cpl["coupled"], keep)
            hs["switched"].couple_tracks(None)
            sample("switched: uncoupled", hs["switched"], cpl["switched"], keep)
            hs["switched"].couple_tracks([1, 0], 1)
            sample("switched: coupled", hs["switched"], cpl["switched"], keep)
        for k, r in rows.items():
            print("| %s | %s | %s | %s | %s |" % (label, k, cell(r["kern"]), cell(r["tick"]), cell(r["full"])))
        a, b = np.median(rows["untracked"]["kern"]), np.median(rows["coupled"]["kern"])
        print("| %s | coupled / untracked rollout kernel | %.4f (agent-steps per launch %d / %d; tracks of %s points) | | |" % (
            label, b / a, np.median(rows["untracked"]["steps"]), np.median(rows["coupled"]["steps"]),
            [len(t) for t in hs["coupled"].get_repulsive_track()]))
        a, b = np.median(rows["switched: uncoupled"]["tick"]), np.median(rows["switched: coupled"]["tick"])
        print("| %s | coupled - uncoupled tick wall, same handle | %.1f us | | |" % (label, b - a))
        sys.stdout.flush()
        for h in hs.values():
            h.close()


if __name__ == "__main__":
    main()
