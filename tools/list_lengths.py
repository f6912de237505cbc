"""Lengths of the ordered force sum's list (circ_and_scale_w64: `count`, the terms K inside the detect shell that are
not skipped) over an episode, replayed on the CPU oracle -- no GPU needed. The one-slot DPP sum adds its list in chunks
of 16 entries: a step with K > 16 runs a second chunk, and the launch lasts as long as the agent with the most of them.

The episode is bench.py's: the oracle ticks with the scene's obstacle list handed to every tick, the real agent put
back at the start every --episode ticks. At every sampled tick the predicted paths are read back and K is counted per
path point from the geometry of the step (sweep of circ_and_scale_w64): field obstacle i counts iff the gate is open,
max(|o_i - p| - (rad + r_i), 1e-5) < shell, and not (ron . gn < -0.01 and ro . rv < -0.01). Velocities are path
differences / dt (the stored paths hold positions only), so the skip test and the gate are approximate near their
thresholds; the obstacles advance along the rollout by their list velocities (at rest in the static configurations).
--dynamic: bench.py's moving-obstacle episode (scenes.advance_live_obstacles after every tick, the start list put back at
every restart). C4 is not modelled: its trailing obstacle is the other arm's set-point, which needs both handles.

usage: python tools/list_lengths.py [--config C2] [--scene 0] [--ticks 256] [--stride 8] [--episode 256] [--runs [--leave-after 8]]
prints the K histogram over all sampled agent-steps and, per sampled tick, the largest per-agent number of steps with
K > 16 and the agent that has it.

--runs: how the long steps lie along a rollout -- what the one-slot kernel's two step loops see (csrc/
pmaf_rollout_w64_body.hpp: the short loop serves the first long step of a run in its rare block, the wave runs the long
loop from the next step on). Per sampled tick, for the agent with the most long steps: the maximal runs of K > 16, and
the steps spent in the long loop / of those with K <= 16 / long steps met in the short loop / loop changes, under
"never leave" and under "leave after R consecutive short steps" (--leave-after R); then the same summed over the
sampled ticks for the per-tick bounding agent and for all agents."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
from oracle.orc import OraclePlanner  # noqa: E402

CHUNK = 16


def step_counts(path, n, sc, init_pos):
    """K per step of one agent: path (cap, 3), n points -> int array of n - 1 counts"""
    if n < 2:
        return np.zeros(0, dtype=np.int64)
    obs = sc["obstacles"][:-1]          # the trailing row is the repulsive-only obstacle
    p = path[:n - 1]
    d = np.diff(path[:n], axis=0) / sc["dt"]
    v = np.vstack([d[:1], d[:-1]])      # velocity going INTO step k (step 0: the first difference)
    gvec = sc["goal"][None, :] - p
    dg = np.linalg.norm(gvec, axis=1)
    gn = gvec / np.where(dg > 0, dg, 1.0)[:, None]
    speed = np.linalg.norm(v, axis=1)
    gate = ~((dg < sc["approach_dist"]) | ((speed < 0.5 * sc["velocity_max"]) &
                                           (np.linalg.norm(p - init_pos[None, :], axis=1) < 0.2)))
    opos = obs[None, :, 0:3] + (np.arange(n - 1) * sc["dt"])[:, None, None] * obs[None, :, 3:6]   # predictObstacles
    ro = opos - p[:, None, :]
    s = np.linalg.norm(ro, axis=2)
    ron = ro / np.where(s > 0, s, 1.0)[:, :, None]
    rv = v[:, None, :] - obs[None, :, 3:6]
    dist = np.maximum(s - (sc.get("radius", 0.05) + obs[None, :, 6]), 1e-5)
    skip = (np.einsum("kmc,kc->km", ron, gn) < -0.01) & (np.einsum("kmc,kmc->km", ro, rv) < -0.01)
    moving = np.einsum("kmc,kmc->km", rv, rv) != 0
    term = (dist < sc["detect_shell_rad"]) & ~skip & moving & gate[:, None]
    return term.sum(axis=1)


def run_stats(k, leave_after=0):
    """k: K per step of one rollout. -> (runs of K > CHUNK, steps in the long loop, of those with K <= CHUNK, long steps
    served by the short loop's rare block, loop changes). The short loop hands over BEHIND a long step; the long loop is
    left behind `leave_after` consecutive short steps (0: never)."""
    lng = np.asarray(k) > CHUNK
    runs = int(lng[0]) + int((lng[1:] & ~lng[:-1]).sum()) if len(lng) else 0
    in_long, short_run = False, 0
    steps_long = short_in_long = long_in_short = changes = 0
    for L in lng:
        if in_long:
            steps_long += 1
            short_in_long += int(not L)
            short_run = 0 if L else short_run + 1
            if leave_after and short_run >= leave_after:
                in_long, short_run = False, 0
                changes += 1
        elif L:
            long_in_short += 1
            in_long, short_run = True, 0
            changes += 1
    return runs, steps_long, short_in_long, long_in_short, changes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scene", type=int, default=0)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--stride", type=int, default=8, help="sample every n-th tick")
    ap.add_argument("--episode", type=int, default=256)
    ap.add_argument("--dynamic", action="store_true", help="moving obstacles, advanced after every tick as bench.py --dynamic does")
    ap.add_argument("--runs", action="store_true", help="report runs of long steps and the long loop's occupancy")
    ap.add_argument("--leave-after", type=int, default=8, help="--runs: R of the rule 'leave after R consecutive short steps'")
    a = ap.parse_args()
    pkg = g.load_package()
    sc = pkg.scenes.config_scene(a.config, a.scene, dynamic=a.dynamic)
    obs0 = sc["obstacles"].copy()
    ora = OraclePlanner(sc, mgr_init_pos=sc["start"])
    n_field = sc["obstacles"].shape[0] - 1
    hist = np.zeros(n_field + 1, dtype=np.int64)
    rows = []
    run_rows = []
    tot_all = np.zeros((2, 5), dtype=np.int64)
    for t in range(a.ticks):
        if a.episode and t % a.episode == 0:
            ora.set_initial_position(sc["start"])
            sc["obstacles"] = obs0.copy()
        elif a.dynamic:
            sc["obstacles"] = pkg.scenes.advance_live_obstacles(sc["obstacles"])
        init_pos = ora.real_state()[0].copy()
        ora.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
        if t % a.stride:
            continue
        paths, n = ora.paths()
        long_steps = np.zeros(sc["n_agents"], dtype=np.int64)
        per_agent = []
        for i in range(sc["n_agents"]):
            k = step_counts(paths[i], int(n[i]), sc, init_pos)
            hist += np.bincount(k, minlength=n_field + 1)
            long_steps[i] = int((k > CHUNK).sum())
            if a.runs:
                st = (run_stats(k), run_stats(k, a.leave_after))
                per_agent.append(st)
                tot_all += np.asarray(st)
        if a.runs:
            i = int(long_steps.argmax())
            run_rows.append((t, int(long_steps[i]), i, per_agent[i]))
        rows.append((t, int(long_steps.max()), int(long_steps.argmax()), int(n.max()) - 1))
    tot = int(hist.sum())
    print("%s%s scene %d: %d ticks, every %d-th sampled, %d agent-steps" % (a.config, " --dynamic" if a.dynamic else "", a.scene, a.ticks, a.stride, tot))
    print("K histogram (terms of the ordered sum per step):")
    for k in np.nonzero(hist)[0]:
        print("  K = %2d  %8d  %5.1f %%" % (k, hist[k], 100.0 * hist[k] / tot))
    over = int(hist[CHUNK + 1:].sum())
    print("steps with K > %d: %d of %d = %.1f %%; largest K %d" % (CHUNK, over, tot, 100.0 * over / max(tot, 1),
                                                                  int(np.nonzero(hist)[0].max())))
    print("tick  most steps with K > %d in one agent (agent)  of steps" % CHUNK)
    for t, m, i, h in rows:
        print("%4d  %4d (agent %2d)  %4d" % (t, m, i, h))
    print("mean over the sampled ticks of the per-launch maximum: %.1f" % np.mean([r[1] for r in rows]))
    if a.runs:
        R = a.leave_after
        print("runs of K > %d along a rollout; per sampled tick the agent with the most long steps" % CHUNK)
        print("tick  long steps (agent)  runs | never leave: in long loop, of those short, long met in short loop, changes"
              " | leave after %d short: the same" % R)
        tot = np.zeros((2, 5), dtype=np.int64)
        for t, m, i, (nv, lv) in run_rows:
            print("%4d  %4d (agent %2d)  %3d | %4d %4d %3d %3d | %4d %4d %3d %3d" % ((t, m, i, nv[0]) + nv[1:] + lv[1:]))
            tot += np.asarray((nv, lv))
        for label, T in (("bounding agents", tot), ("all agents", tot_all)):
            for rule, r in zip(("never leave", "leave after %d" % R), T):
                # (a short-list step costs the long loop 22 issue slots of ~460: profiles/c2_long_loop.md section 3)
                print("%s, %s: %d steps in the long loop, %d of them short (%.1f %%: at 22 issue slots of ~460 each "
                      "%.2f %% of those steps' time), %d long steps served by the short loop, %d loop changes"
                      % (label, rule, r[1], r[2], 100.0 * r[2] / max(r[1], 1), 100.0 * 22 / 460 * r[2] / max(r[1], 1), r[3], r[4]))
    ora.close()


if __name__ == "__main__":
    main()
