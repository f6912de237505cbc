"""Time of the clear selection against the obstacle tracks (pmaf_select_clear_tracked) next to the figure it is to be
judged by, one handle per configuration, all in one process on one box:
  untracked   pmaf_select_clear (adopt = 0) on the same handle: unchanged code, the yardstick;
  tracked     pmaf_select_clear_tracked (adopt = 0) against attached tracks of cap + 5 points (the live list's straight
              lines with a drift on every obstacle, so no two points are equal), offset 1,
each at horizon = cap and at horizon = 50. HIP events on the handle's stream around each side (the stream is idle: every
sample follows a drained tick and one pmaf_evaluate), the host's wall clock around the same calls beside them. --warmup
calls, then the median of --calls, the sides interleaved sample by sample; min .. max is the run-to-run spread the tool
reports. Configurations whose rollout kernel cannot follow tracks (more than 60 field obstacles) are refused by
pmaf_set_obstacle_tracks.
usage: python tools/tracked_audit_time.py [--calls 20] [--warmup 5] [C2 C1 ...]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def drifting_lines(obs, dt, n):
    """[n][M][6]: the iterated straight lines of the field obstacles of `obs`, each with a slow drift of its own"""
    o = np.asarray(obs, dtype=np.float64)[:-1]
    out = np.zeros((n, len(o), 6))
    q = o[:, 0:3].copy()
    for k in range(n):
        out[k, :, 0:3] = q + 0.0004 * k * np.cos(np.arange(len(o))[:, None] + np.arange(3)[None, :])
        out[k, :, 3:6] = o[:, 3:6]
        q = q + o[:, 3:6] * dt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C2", "C1"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
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

    def row(name, v):
        v = np.asarray(v)
        return "%-30s median %8.1f  min %8.1f  max %8.1f us" % (name, np.median(v), v.min(), v.max())

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
        tracks = [drifting_lines(live[p], sc["dt"], h.cap + 5) for p in range(P)]
        h.set_obstacle_tracks(tracks[0] if P == 1 else tracks)
        h.set_obstacle_track_offset(1)
        stream = C.c_void_p(h.stream())
        sides = {}
        for hname, horizon in (("cap", h.cap), ("50", 50)):
            sides["untracked horizon=" + hname] = lambda horizon=horizon: h.select_clear(live, 0.05, horizon)
            sides["tracked   horizon=" + hname] = lambda horizon=horizon: h.select_clear_tracked(live, 0.05, horizon)
        dev = {k: [] for k in sides}
        wall = {k: [] for k in sides}
        last = {}
        h.start()
        for it in range(args.warmup + args.calls):
            h.stop()
            h.evaluate(sc["cost_gains"], sc["ws_limits"])
            for k, fn in sides.items():      # interleaved: every sample of every side sees the same rollout
                out, d_us, w_us = timed(stream, fn)
                assert np.all(np.asarray(out["pick"]) >= 0)
                last[k] = out
                if it >= args.warmup:
                    dev[k].append(d_us)
                    wall[k].append(w_us)
            best = np.asarray(h.evaluate(sc["cost_gains"], sc["ws_limits"]))
            h.move_real(obs, sc["dt"], 1, best)
            pos, vel, _ = h.real_state()
            h.reset_agents(pos, vel, obs)
            h.start()
        h.stop()
        print("%s: %d x %d agents, cap %d, %d obstacles, tracks of %d points" % (cfg, P, h.N, h.cap, h.n_obs, h.cap + 5))
        for k in sides:
            print("  device  " + row(k, dev[k]) + "   n_clear %s" % np.asarray(last[k]["n_clear"]).tolist())
        for k in sides:
            print("  wall    " + row(k, wall[k]))
        for hname in ("cap", "50"):
            u, t = np.asarray(dev["untracked horizon=" + hname]), np.asarray(dev["tracked   horizon=" + hname])
            print("  ratio   tracked / untracked at horizon=%s: %.3f of the medians (untracked spread %.1f %%, tracked %.1f %%)" % (
                hname, np.median(t) / np.median(u), 100.0 * (u.max() - u.min()) / np.median(u),
                100.0 * (t.max() - t.min()) / np.median(t)))
        h.close()


if __name__ == "__main__":
    main()
