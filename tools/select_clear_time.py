"""Time of the selection against the live list (pmaf_select_clear) next to the figure it is to be judged by, one handle per
configuration, all in one process on one box:
  yardstick   today's way to the same answer on the same handle: pmaf_evaluate_paths (lean call: clearance and
              first_violation only) + pmaf_get_costs, the rule then being the caller's;
  select      pmaf_select_clear (adopt = 0) at horizon = cap and at horizon = 50.
HIP events on the handle's stream around each side (the stream is idle: every sample follows a drained tick and one
pmaf_evaluate), the host's wall clock around the same calls beside them. --warmup calls, then the median of --calls, the
sides interleaved sample by sample; min .. max is the run-to-run spread the tool reports.
  ticks       host wall clock of the node's five calls (stop, evaluate, move_real, reset_agents, start) and of the
              six-call audited tick (select_clear(adopt = 1) behind evaluate), the stream drained in front of each, and
              pmaf_tick's own clock (pmaf_get_tick_times_us: set-point on the host) for the fused tick.
usage: python tools/select_clear_time.py [--calls 20] [--warmup 5] [C2 C3 C5x8 ...]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


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
        return "%-28s median %8.1f  min %8.1f  max %8.1f us" % (name, np.median(v), v.min(), v.max())

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
        stream = C.c_void_p(h.stream())
        sides = {"yardstick": lambda: (h.evaluate_paths(live, 0.05), h.costs()),
                 "select horizon=cap": lambda: h.select_clear(live, 0.05, h.cap),
                 "select horizon=50": lambda: h.select_clear(live, 0.05, 50)}
        dev = {k: [] for k in sides}
        wall = {k: [] for k in sides}
        picks = None
        h.start()
        for it in range(args.warmup + args.calls):
            h.stop()
            h.evaluate(sc["cost_gains"], sc["ws_limits"])
            for k, fn in sides.items():      # interleaved: every sample of every side sees the same rollout
                out, d_us, w_us = timed(stream, fn)
                if it >= args.warmup:
                    dev[k].append(d_us)
                    wall[k].append(w_us)
                if k == "select horizon=cap":
                    picks = out
                    # the same answer the yardstick's outputs give under the caller's own rule
                    assert np.all(np.asarray(out["pick"]) >= 0)
            best = np.asarray(h.evaluate(sc["cost_gains"], sc["ws_limits"]))
            h.move_real(obs, sc["dt"], 1, best)
            pos, vel, _ = h.real_state()
            h.reset_agents(pos, vel, obs)
            h.start()
        h.stop()
        # the node's five calls and the audited tick's six, host wall clock, the stream drained in front of each
        five, six = [], []
        prev = None
        for it in range(args.warmup + args.calls):
            for which in ("five", "six"):
                h.stop()
                t0 = time.perf_counter()
                if which == "five":
                    h.stop()
                    best = np.asarray(h.evaluate(sc["cost_gains"], sc["ws_limits"]))
                    h.move_real(obs, sc["dt"], 1, best)
                    pos, vel, _ = h.real_state()
                    h.reset_agents(pos, vel, obs)
                    h.start()
                else:
                    prev = h.audited_tick(live, sc["dt"], sc["cost_gains"], sc["ws_limits"], 0.05, h.cap, prev=prev)["pick"]
                us = (time.perf_counter() - t0) * 1e6
                if it >= args.warmup:
                    (five if which == "five" else six).append(us)
        h.stop()
        h.tick_times_us()
        for it in range(args.warmup + args.calls):
            h.stop()
            h.tick(obs, sc["dt"], sc["cost_gains"], sc["ws_limits"])
        h.stop()
        _, sp = h.tick_times_us()
        print("%s: %d x %d agents, cap %d, %d obstacles | last select %s" % (
            cfg, P, h.N, h.cap, h.n_obs, {k: np.asarray(v).tolist() for k, v in picks.items() if k in ("pick", "rule", "n_clear")}
            if P <= 2 else {"rule": np.asarray(picks["rule"]).tolist()}))
        for k in sides:
            print("  device  " + row(k, dev[k]))
        for k in sides:
            print("  wall    " + row(k, wall[k]))
        print("  tick    " + row("five calls", five))
        print("  tick    " + row("six calls (audited)", six))
        print("  tick    " + row("pmaf_tick set-point", sp[args.warmup:]))
        h.close()


if __name__ == "__main__":
    main()
