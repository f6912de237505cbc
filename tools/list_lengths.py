"""Lengths of the ordered force sum's list (circ_and_scale_w64: `count`, the terms K inside the detect shell that are
not skipped) over an episode, replayed on the CPU oracle -- no GPU needed. The one-slot DPP sum adds its list in chunks
of 16 entries: a step with K > 16 runs a second chunk, and the launch lasts as long as the agent with the most of them.

The episode is bench.py's: the oracle ticks with the scene's obstacle list handed to every tick, the real agent put
back at the start every --episode ticks. At every sampled tick the predicted paths are read back and K is counted per
path point from the geometry of the step (sweep of circ_and_scale_w64): field obstacle i counts iff the gate is open,
max(|o_i - p| - (rad + r_i), 1e-5) < shell, and not (ron . gn < -0.01 and ro . rv < -0.01). Velocities are path
differences / dt (the stored paths hold positions only), so the skip test and the gate are approximate near their
thresholds; obstacles are taken at rest at their tick positions (static configurations).

usage: python tools/list_lengths.py [--config C2] [--scene 0] [--ticks 256] [--stride 8] [--episode 256]
prints the K histogram over all sampled agent-steps and, per sampled tick, the largest per-agent number of steps with
K > 16 and the agent that has it."""
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
    ro = obs[None, :, 0:3] - p[:, None, :]
    s = np.linalg.norm(ro, axis=2)
    ron = ro / np.where(s > 0, s, 1.0)[:, :, None]
    rv = v[:, None, :] - obs[None, :, 3:6]
    dist = np.maximum(s - (sc.get("radius", 0.05) + obs[None, :, 6]), 1e-5)
    skip = (np.einsum("kmc,kc->km", ron, gn) < -0.01) & (np.einsum("kmc,kmc->km", ro, rv) < -0.01)
    moving = np.einsum("kmc,kmc->km", rv, rv) != 0
    term = (dist < sc["detect_shell_rad"]) & ~skip & moving & gate[:, None]
    return term.sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scene", type=int, default=0)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--stride", type=int, default=8, help="sample every n-th tick")
    ap.add_argument("--episode", type=int, default=256)
    a = ap.parse_args()
    pkg = g.load_package()
    sc = pkg.scenes.config_scene(a.config, a.scene)
    ora = OraclePlanner(sc, mgr_init_pos=sc["start"])
    n_field = sc["obstacles"].shape[0] - 1
    hist = np.zeros(n_field + 1, dtype=np.int64)
    rows = []
    for t in range(a.ticks):
        if a.episode and t % a.episode == 0:
            ora.set_initial_position(sc["start"])
        init_pos = ora.real_state()[0].copy()
        ora.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
        if t % a.stride:
            continue
        paths, n = ora.paths()
        long_steps = np.zeros(sc["n_agents"], dtype=np.int64)
        for i in range(sc["n_agents"]):
            k = step_counts(paths[i], int(n[i]), sc, init_pos)
            hist += np.bincount(k, minlength=n_field + 1)
            long_steps[i] = int((k > CHUNK).sum())
        rows.append((t, int(long_steps.max()), int(long_steps.argmax()), int(n.max()) - 1))
    tot = int(hist.sum())
    print("%s scene %d: %d ticks, every %d-th sampled, %d agent-steps" % (a.config, a.scene, a.ticks, a.stride, tot))
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
    ora.close()


if __name__ == "__main__":
    main()
