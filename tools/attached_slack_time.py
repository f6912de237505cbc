"""Time of the joint selection on coupled handles with timing slack (pmaf_cross_audit_attached_slack /
pmaf_select_pair_clear_tracked_slack) next to the figures it is to be judged by, at C4's shape (2 x 256 agents, --columns
attached columns per side: 1 + 2 * columns terms), for each slack of --slacks, all in one process on one box:
  audit        pmaf_cross_audit_slack at the same slack (k_cross_audit_slack, unchanged code: the yardstick, one term)
               against pmaf_cross_audit_attached_slack on the coupled handle (k_xaudit_attached_slack, every term) and
               on an uncoupled handle (term 0 alone); at (0, 0) also pmaf_cross_audit_attached on the coupled handle
               (k_cross_audit_attached: the same answer through the un-slacked kernel). Every call downloads its
               256 x 256 matrix, the attached ones also upload the list.
  joint        pmaf_select_pair_clear_tracked_slack on the coupled handle against what a caller has to do today for the
               same answer, the host's rule not timed: pmaf_select_clear_tracked(skip_trailing), pmaf_cross_audit_slack
               for term 0, one pmaf_cross_audit_tracks_slack per sphere term on sphere paths composed on the host (outside
               the timed region; for a term 1 + M + s the populations' roles and the two slacks are exchanged) and
               pmaf_get_costs
HIP events on the handles' streams around each side (the stream is idle: every sample follows a drained tick and one
pmaf_evaluate), the host's wall clock beside them. --warmup calls, then the median of --calls, the sides interleaved
sample by sample; min .. max is the run-to-run spread the tool reports.
usage: python tools/attached_slack_time.py [--calls 20] [--warmup 5] [--columns 4] [--slacks 0,0:5,5:30,30] [--md FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

SEP = 0.15


def cell(v):
    v = np.asarray(v)
    return "%.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def spread(v):
    v = np.asarray(v)
    return (v.max() - v.min()) / np.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--columns", type=int, default=4)
    ap.add_argument("--slacks", default="0,0:5,5:30,30")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    slacks = [tuple(int(v) for v in s.split(",")) for s in args.slacks.split(":")]
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

    arms = pm.scenes.dual_arm_scenes()      # C4: 2 x 256 agents
    sc = arms[0]
    starts = np.stack([s["start"] for s in arms])
    obs = np.stack([s["obstacles"] for s in arms])
    live = np.stack([pm.scenes.advance_live_obstacles(o) for o in obs])
    M, n_col = obs.shape[1] - 1, args.columns
    src = np.full((2, M), -1, dtype=np.int32)
    scale = np.ones((2, M))
    anchor = np.zeros((2, M, 3))
    for c in range(n_col):      # gripper, load and forearm spheres: scales 1 .. 0.7, anchors a few centimetres off
        src[0, c], src[1, c] = 1, 0
        scale[:, c] = 1.0 - 0.1 * c
        anchor[:, c] = 0.1 * c * starts.mean(axis=0) + np.array([0.02 * c, -0.03, 0.01 * c])
    n_terms = 1 + 2 * n_col
    hs = {}
    for name in ("coupled", "uncoupled"):
        h = pm.PmafPlanner(arms, device=0, mgr_init_pos=starts)
        h.set_initial_position(starts)
        if name == "coupled":
            h.couple_obstacle_tracks(src, scale, anchor, 1)
        h.start()
        hs[name] = h
    hc, hu = hs["coupled"], hs["uncoupled"]
    N, cap = hc.N, hc.cap
    horizon = cap
    state = {}

    def today(la, lb):
        """the same answer with the calls that exist without this one: the host composes every sphere term's paths (done
        in refresh(), not timed), the device audits them one launch per term"""
        sel = hc.select_clear_tracked(live, 0.03, horizon, skip_trailing=True)
        mats = [hc.cross_audit_slack(0, 1, SEP, la, lb)]
        for pop, tracks, n in state["terms"]:
            # pop 0 against spheres on arm 1's paths: k is arm 0's step; pop 1 against spheres on arm 0's: the roles of
            # A and B, and with them the two slacks, are exchanged
            mats.append(hc.cross_audit_tracks_slack(pop, tracks, n, SEP, la if pop == 0 else lb, lb if pop == 0 else la))
        return sel, mats, hc.costs()

    def refresh():
        paths, n = hc.paths()
        paths, n = np.asarray(paths).reshape(2, N, cap, 3), np.asarray(n).reshape(2, N).astype(np.int32)
        terms = []
        for p in (0, 1):
            for c in range(n_col):
                terms.append((p, anchor[p, c][None, None, :] + scale[p, c] * paths[1 - p], n[1 - p]))
        state["terms"] = terms

    sides = {}
    for la, lb in slacks:
        tag = "(%d, %d)" % (la, lb)
        sides["audit %s pmaf_cross_audit_slack" % tag] = (hu, lambda la=la, lb=lb: hu.cross_audit_slack(0, 1, SEP, la, lb))
        sides["audit %s attached_slack, term 0 alone" % tag] = (
            hu, lambda la=la, lb=lb: hu.cross_audit_attached_slack(0, 1, live, SEP, la, lb))
        sides["audit %s attached_slack, %d terms" % (tag, n_terms)] = (
            hc, lambda la=la, lb=lb: hc.cross_audit_attached_slack(0, 1, live, SEP, la, lb))
        if (la, lb) == (0, 0):
            sides["audit %s pmaf_cross_audit_attached, %d terms" % (tag, n_terms)] = (
                hc, lambda: hc.cross_audit_attached(0, 1, live, SEP))
        sides["joint %s today: %d calls" % (tag, n_terms + 2)] = (hc, lambda la=la, lb=lb: today(la, lb))
        sides["joint %s select_pair_clear_tracked_slack" % tag] = (
            hc, lambda la=la, lb=lb: hc.select_pair_clear_tracked(0, 1, live, 0.03, horizon, SEP, 0.02, skip_trailing=True,
                                                                   late=(la, lb)))
    dev = {k: [] for k in sides}
    wall = {k: [] for k in sides}
    for it in range(args.warmup + args.calls):
        for h in (hc, hu):
            h.stop()
            h.evaluate(sc["cost_gains"], sc["ws_limits"])
        refresh()
        for k, (h, fn) in sides.items():      # interleaved: every sample of every side sees a finished rollout
            _, d_us, w_us = timed(C.c_void_p(h.stream()), fn)
            if it >= args.warmup:
                dev[k].append(d_us)
                wall[k].append(w_us)
        for h in (hc, hu):
            best = np.asarray(h.evaluate(sc["cost_gains"], sc["ws_limits"]))
            h.move_real(obs, sc["dt"], 1, best)
            pos, vel, _ = h.real_state()
            h.reset_agents(pos, vel, obs)
            h.start()
    for h in (hc, hu):
        h.stop()
        h.close()
    lines = ["C4: 2 x %d agents, cap %d, %d obstacles, %d attached columns per side (%d terms); median of %d (min .. max), us"
             % (N, cap, M + 1, n_col, n_terms, args.calls), "",
             "| side | device (HIP events) | host wall clock |", "|---|---|---|"]
    for k in sides:
        lines.append("| %s | %s | %s |" % (k, cell(dev[k]), cell(wall[k])))
    med = {k: float(np.median(dev[k])) for k in sides}
    lines.append("")
    for la, lb in slacks:
        tag = "(%d, %d)" % (la, lb)
        y = "audit %s pmaf_cross_audit_slack" % tag
        x = "audit %s attached_slack, %d terms" % (tag, n_terms)
        lines.append("* %s attached_slack of %d terms / (%d x pmaf_cross_audit_slack): %.3f; term 0 alone / pmaf_cross_audit_slack: "
                     "%.3f (yardstick spread %.1f %%; both sides hold one matrix download, the attached one also the list's upload)"
                     % (tag, n_terms, n_terms, med[x] / (n_terms * med[y]),
                        med["audit %s attached_slack, term 0 alone" % tag] / med[y], 100 * spread(dev[y])))
        if (la, lb) == (0, 0):
            lines.append("* (0, 0) attached_slack / pmaf_cross_audit_attached, %d terms each: %.3f"
                         % (n_terms, med[x] / med["audit %s pmaf_cross_audit_attached, %d terms" % (tag, n_terms)]))
        td = "joint %s today: %d calls" % (tag, n_terms + 2)
        lines.append("* %s joint call / today's calls: %.3f (today's spread %.1f %%)"
                     % (tag, med["joint %s select_pair_clear_tracked_slack" % tag] / med[td], 100 * spread(dev[td])))
    text = "\n".join(lines)
    print(text)
    if args.md:
        with open(args.md, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
