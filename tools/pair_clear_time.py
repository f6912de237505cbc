"""Time of the joint selection (pmaf_select_pair_clear) next to the figures it is to be judged by, one handle per row, all
in one process on one box:
  yardstick   the way to the same inputs on the same handle without the call: pmaf_evaluate_paths (lean call: clearance
              and first_violation only) + pmaf_cross_audit (or _slack) with the N x N matrix copied out + pmaf_get_costs;
              the host's numpy rule is NOT timed, which favours the yardstick;
  joint       pmaf_select_pair_clear (adopt = 0, skip_trailing = 1) at horizon = cap and at horizon = 50;
  alone       pmaf_select_clear and pmaf_select_pair (or _slack), the two stand-alone calls, and their sum per sample.
Rows: C4 (2 x 256 agents x 200 steps x 32 obstacles) and 2 x 1024 x 200 x 32 step against step, C4 at +-30 steps of slack.
HIP events on the handle's stream around each side (the stream is idle: every sample follows a drained tick and one
pmaf_evaluate), the host's wall clock around the same calls beside them. --warmup calls, then the median of --calls with
min .. max (the run-to-run spread), the sides interleaved sample by sample. Prints a markdown table (profiles/
select_pair_clear.md keeps one run's output).
usage: python tools/pair_clear_time.py [--calls 20] [--warmup 5]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

SEP, OM, PM = 0.15, 0.05, 0.02


def main():
    ap = argparse.ArgumentParser()
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

    def cell(v):
        v = np.asarray(v)
        return "%.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())

    print("| row | side | device us: median (min .. max) | host wall us: median (min .. max) |")
    print("|---|---|---|---|")
    for label, n_agents, late in (("C4 2 x 256 x 200 x 32", 256, None), ("2 x 1024 x 200 x 32", 1024, None),
                                  ("C4, slack +-30 steps", 256, (30, 30))):
        arms = pm.scenes.dual_arm_scenes(n_agents=n_agents)
        sc = arms[0]
        starts = np.stack([s["start"] for s in arms])
        h = pm.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        h.set_initial_position(starts)
        cpl = pm.shard.DualArmCoupling(np.stack([s["obstacles"] for s in arms]), 0.1)
        stream = C.c_void_p(h.stream())
        state = {}

        def audit():
            if late is None:
                return h.cross_audit(0, 1, SEP)
            return h.cross_audit_slack(0, 1, SEP, late[0], late[1])

        def pair():
            if late is None:
                return h.select_pair(0, 1, SEP, PM)
            return h.select_pair_slack(0, 1, SEP, PM, late[0], late[1])

        def alone():
            return h.select_clear(state["live"], OM, h.cap), pair()

        sides = {"yardstick: evaluate_paths + cross_audit (matrix out) + get_costs":
                 lambda: (h.evaluate_paths(state["live"], OM), audit(), h.costs()),
                 "select_pair_clear horizon=cap": lambda: h.select_pair_clear(0, 1, state["live"], OM, h.cap, SEP, PM,
                                                                              skip_trailing=True, late=late),
                 "select_pair_clear horizon=50": lambda: h.select_pair_clear(0, 1, state["live"], OM, 50, SEP, PM,
                                                                             skip_trailing=True, late=late),
                 "select_clear alone": lambda: h.select_clear(state["live"], OM, h.cap),
                 "select_pair%s alone" % ("" if late is None else "_slack"): pair,
                 "sum of the two stand-alone calls": alone}
        dev = {k: [] for k in sides}
        wall = {k: [] for k in sides}
        last = None
        h.start()
        for it in range(args.warmup + args.calls):
            h.stop()
            best = np.asarray(h.evaluate(sc["cost_gains"], sc["ws_limits"]))
            obs = cpl.coupled_obstacles(h.real_state()[0])
            state["live"] = obs
            for k, fn in sides.items():      # interleaved: every sample of every side sees the same rollout
                out, d_us, w_us = timed(stream, fn)
                if it >= args.warmup:
                    dev[k].append(d_us)
                    wall[k].append(w_us)
                if k == "select_pair_clear horizon=cap":
                    last = out
            h.move_real(obs, sc["dt"], 1, best)
            pos, vel, _ = h.real_state()
            h.reset_agents(pos, vel, obs)
            h.start()
        h.stop()
        for k in sides:
            print("| %s | %s | %s | %s |" % (label, k, cell(dev[k]), cell(wall[k])))
        print("| %s | last joint result | rule %d, n_feasible %d, n_clear %s, pair %s | |" % (
            label, last["rule"], last["n_feasible"], last["n_clear"], last["pair"]))
        sys.stdout.flush()
        h.close()


if __name__ == "__main__":
    main()
