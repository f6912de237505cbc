"""Time of the joint selection on coupled handles (pmaf_cross_audit_attached / pmaf_select_pair_clear_tracked) next to
the figures it is to be judged by, at C4's shape (2 x 256 agents), all in one process on one box:
  audit        pmaf_cross_audit (k_cross_audit, unchanged code: the yardstick) against pmaf_cross_audit_attached on a
               handle with --columns attached columns per side (k_cross_audit_attached, 1 + 2 * columns terms) and on an
               uncoupled handle (term 0 alone); every call downloads its 256 x 256 matrix, the attached ones also upload
               the list
  joint        pmaf_select_pair_clear_tracked on the coupled handle against what a caller has to do today for the same
               answer, the host's rule not timed: pmaf_select_clear_tracked(skip_trailing), one pmaf_cross_audit_tracks
               per term on sphere paths composed on the host (outside the timed region) and pmaf_get_costs
  plain        pmaf_select_pair_clear_tracked against pmaf_select_pair_clear(late = NULL) on the uncoupled handle
HIP events on the handles' streams around each side (the stream is idle: every sample follows a drained tick and one
pmaf_evaluate), the host's wall clock beside them. --warmup calls, then the median of --calls, the sides interleaved
sample by sample; min .. max is the run-to-run spread the tool reports.
  with --trace DIR: the durations of k_cross_audit and k_cross_audit_attached out of a kernel trace of THIS script
  (rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/attached_audit_time.py): the kernels alone,
  without the copies around them; the attached kernel's dispatches are split by its grid's terms (coupled / uncoupled
  handle) in the order the script issues them.
usage: python tools/attached_audit_time.py [--calls 20] [--warmup 5] [--columns 4] [--md FILE] | --trace DIR"""
import argparse
import csv
import ctypes as C
import glob
import os
import re
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


def trace(directory, calls):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under " + directory
    # (the trace names a kernel mangled or demangled, depending on the profiler's version)
    dur = {"k_cross_audit_attached": [], "k_cross_auditE": []}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"]
            k = "k_cross_audit_attached" if "k_cross_audit_attached" in name else (
                "k_cross_auditE" if re.search(r"k_cross_audit(E|\(|$)", name) else None)
            if k:
                dur[k].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3))
    print("| kernel | dispatches in the trace | device us: median (min .. max) |")
    print("|---|---|---|")
    plain = [d for _, d in sorted(dur["k_cross_auditE"])]
    att = [d for _, d in sorted(dur["k_cross_audit_attached"])]
    print("| k_cross_audit | %d | %s |" % (len(plain), cell(plain[-calls:])))
    # two populations of durations: the uncoupled handle's term 0 alone and the coupled handle's terms
    cut = 2.0 * np.median(plain)
    for name, v in (("k_cross_audit_attached, term 0 alone", [d for d in att if d < cut]),
                    ("k_cross_audit_attached, every term", [d for d in att if d >= cut])):
        if v:
            print("| %s | %d | %s |" % (name, len(v), cell(v[-calls:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--columns", type=int, default=4)
    ap.add_argument("--md", default=None)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        return trace(args.trace, args.calls)
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

    def today():
        """the same answer with the calls that exist without this one: the host composes every term's sphere paths
        (done in refresh(), not timed), the device audits them one launch per term"""
        sel = hc.select_clear_tracked(live, 0.03, horizon, skip_trailing=True)
        mats = [hc.cross_audit(0, 1, SEP)]
        for pop, tracks, n in state["terms"]:
            mats.append(hc.cross_audit_tracks(pop, tracks, n, SEP))
        return sel, mats, hc.costs()

    def refresh():
        paths, n = hc.paths()
        paths, n = np.asarray(paths).reshape(2, N, cap, 3), np.asarray(n).reshape(2, N).astype(np.int32)
        terms = []
        for p in (0, 1):
            for c in range(n_col):
                terms.append((p, anchor[p, c][None, None, :] + scale[p, c] * paths[1 - p], n[1 - p]))
        state["terms"] = terms

    sides = {
        "audit  pmaf_cross_audit": (hu, lambda: hu.cross_audit(0, 1, SEP)),
        "audit  attached, term 0 alone": (hu, lambda: hu.cross_audit_attached(0, 1, live, SEP)),
        "audit  attached, %d terms" % n_terms: (hc, lambda: hc.cross_audit_attached(0, 1, live, SEP)),
        "joint  today: %d calls" % (n_terms + 2): (hc, today),
        "joint  select_pair_clear_tracked": (hc, lambda: hc.select_pair_clear_tracked(0, 1, live, 0.03, horizon, SEP, 0.02,
                                                                                        skip_trailing=True)),
        "plain  select_pair_clear": (hu, lambda: hu.select_pair_clear(0, 1, live, 0.03, horizon, SEP, 0.02, skip_trailing=True)),
        "plain  select_pair_clear_tracked": (hu, lambda: hu.select_pair_clear_tracked(0, 1, live, 0.03, horizon, SEP, 0.02,
                                                                                        skip_trailing=True)),
    }
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
    names = list(sides)
    lines = ["C4: 2 x %d agents, cap %d, %d obstacles, %d attached columns per side (%d terms); median of %d (min .. max), us"
             % (N, cap, M + 1, n_col, n_terms, args.calls), "",
             "| side | device (HIP events) | host wall clock |", "|---|---|---|"]
    for k in names:
        lines.append("| %s | %s | %s |" % (k, cell(dev[k]), cell(wall[k])))
    med = {k: float(np.median(dev[k])) for k in names}
    a, x0, x9, td, jt, pp, pt = names
    lines += ["",
              "* attached audit of %d terms / (%d x pmaf_cross_audit): %.3f (yardstick spread %.1f %%; both sides hold one "
              "matrix download, the attached one also the list's upload)" % (n_terms, n_terms, med[x9] / (n_terms * med[a]), 100 * spread(dev[a])),
              "* attached audit, term 0 alone / pmaf_cross_audit: %.3f" % (med[x0] / med[a]),
              "* joint call / today's calls: %.3f (today's spread %.1f %%)" % (med[jt] / med[td], 100 * spread(dev[td])),
              "* no attachments, tracked / untracked joint call: %.3f (untracked spread %.1f %%)" % (med[pt] / med[pp], 100 * spread(dev[pp]))]
    text = "\n".join(lines)
    print(text)
    if args.md:
        with open(args.md, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
