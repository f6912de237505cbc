"""Time of the path audit (pmaf_evaluate_paths) next to the two figures it is to be judged by, per configuration:
  audit     HIP events on the handle's stream around one pmaf_evaluate_paths call after the rollout has finished
            (obstacle upload, k_audit_track, k_path_audit, one device-to-host copy of the results); also the host's
            wall clock around the same call (what the caller waits);
  rollout   the same handle's rollout kernel, pmaf_get_kernel_stats (HIP events on its dispatch);
  host      today's alternative: pmaf_get_paths (the copy of all paths of that rollout) + the reference loop
            vectorised in numpy, host wall clock.
Median of --calls calls after --warmup; every call audits a fresh rollout (one tick in front of it, drained).
usage: python tools/path_audit_time.py [--calls 20] [--warmup 5] [C2 C3 C5x8 ...]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def host_audit(paths, n_points, obstacles, dt, rad, right_assoc, chunk=32):
    """the reference loop in numpy for one population: clearance [N] (min over the valid points and all obstacles)"""
    N, cap, _ = paths.shape
    pos, vel = obstacles[:, 0:3].copy(), obstacles[:, 3:6]
    track = np.empty((cap, obstacles.shape[0], 3))
    for k in range(cap):
        track[k] = pos
        pos = pos + vel * dt
    rr = rad + obstacles[:, 6]
    out = np.empty(N)
    for a0 in range(0, N, chunk):
        d = paths[a0:a0 + chunk, :, None, :] - track[None]
        sq = d * d
        s = sq[..., 0] + (sq[..., 1] + sq[..., 2]) if right_assoc else (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        c = np.sqrt(s) - rr
        valid = np.arange(cap)[None, :, None] < n_points[a0:a0 + chunk, None, None]
        out[a0:a0 + chunk] = np.where(valid, c, np.inf).min(axis=(1, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C2", "C3", "C5x8"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    pm = g.load_package()
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    order = pm.load_library().pmaf_eval_order()
    for cfg in args.configs:
        name, _, reps = cfg.partition("x")
        P = int(reps or 1)
        scs = [pm.scenes.config_scene(name, scene_id=p) for p in range(P)]
        sc = scs[0]
        starts = np.stack([s["start"] for s in scs])
        obs = np.stack([s["obstacles"] for s in scs])
        live = np.stack([pm.scenes.advance_live_obstacles(o) for o in obs])
        h = pm.PmafPlanner(scs, device=0, mgr_init_pos=starts)
        h.set_initial_position(starts)
        h.set_profiling(True)
        stream = C.c_void_p(h.stream())
        dev_ms, wall_us, host_us = [], [], []
        for it in range(args.warmup + args.calls):
            if it == args.warmup:
                h.stop()
                h.reset_kernel_stats()
            h.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
            h.stop()
            assert hip.hipEventRecord(ev[0], stream) == 0
            t0 = time.perf_counter()
            got = h.evaluate_paths(live, 0.05)
            t1 = time.perf_counter()
            assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
            t2 = time.perf_counter()
            paths, n = h.paths()
            paths, n = paths.reshape(P, h.N, h.cap, 3), n.reshape(P, h.N)
            ref = np.stack([host_audit(paths[p], n[p], live[p], sc["dt"], sc.get("radius", 0.05), order) for p in range(P)])
            t3 = time.perf_counter()
            if it >= args.warmup:
                dev_ms.append(ms.value); wall_us.append((t1 - t0) * 1e6); host_us.append((t3 - t2) * 1e6)
            assert (np.asarray(got["clearance"]).reshape(P, h.N) == ref).all(), "the audit and the numpy loop disagree"
        h.stop()
        ms, launches, _ = h.kernel_stats()
        pairs = int(n.sum()) * h.n_obs
        print("%s: P %d N %d cap %d n_obs %d, %.1f M pairs | audit %.1f us (events; caller's wall clock %.1f us) | rollout kernel "
              "%.1f us | get_paths + numpy loop %.0f us | median of %d calls" %
              (cfg, P, h.N, h.cap, h.n_obs, pairs / 1e6, np.median(dev_ms) * 1e3, np.median(wall_us),
               ms / max(launches, 1) * 1e3, np.median(host_us), args.calls), flush=True)
        h.close()


if __name__ == "__main__":
    main()
