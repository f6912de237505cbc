"""The joint selection (pmaf_select_pair_clear / pmaf_select_clear_tracks), the parts that need no GPU: the reference the
GPU suite compares with (tests/pair_clear_reference.py) against a brute-force restatement, six mutants that hand cases
must catch, the parametrisation of the GPU shapes on the oracle's rollouts (tests/pair_clear_cases.py: the oracle's paths
are the GPU's, bit for bit) with what it has to reach, the binding table, the header, the resource record and the C++
facade through a compiler."""
import os
import random
import subprocess

import numpy as np
import pytest

import conftest
import cross_audit_reference as car
import pair_clear_cases as pc
import pair_clear_reference as ref
import select_clear_reference as scr

ROOT = conftest.ROOT
INF = float("inf")
NAN = float("nan")


# ---- the reference against a brute-force restatement: sets and sorts instead of scans ----
def _brute(cost_a, cost_b, clear_a, clear_b, c_a, c_b, clearance, om, pm, prev):
    na, nb = len(cost_a), len(cost_b)
    pairs = [(i, j) for i in range(na) for j in range(nb)]
    feas = {(i, j) for i, j in pairs if clear_a[i] and clear_b[j] and clearance[i][j] >= pm}
    total = {(i, j): cost_a[i] + cost_b[j] for i, j in pairs}
    comparable = sorted((total[q], q[0], q[1]) for q in feas if total[q] < INF)
    if comparable:
        s, i, j = comparable[0]
        if prev is not None and prev[0] >= 0 and prev[1] >= 0 and tuple(prev) in feas and s >= 0.9 * total[tuple(prev)]:
            return tuple(prev), 0, len(feas)
        return (i, j), 1, len(feas)
    g = {}
    for i, j in pairs:
        terms = [c_a[i] - om] + ([] if c_b is None else [c_b[j] - om]) + [clearance[i][j] - pm]
        if terms[-1] != terms[-1]:
            continue
        g[(i, j)] = min(terms)
    ranked = sorted((-v, q[0], q[1]) for q, v in g.items() if v > -INF)
    if ranked:
        return (ranked[0][1], ranked[0][2]), 2, len(feas)
    return (-1, -1), -1, len(feas)


def _random_tables(rng, na, nb, tracks):
    pool = [1.0, 2.0, 2.0, 3.5, 0.25, INF, NAN]
    cost_a = [rng.choice(pool) for _ in range(na)]
    cost_b = [rng.choice(pool[:5]) for _ in range(nb)]
    clear_a = [rng.random() < 0.6 for _ in range(na)]
    clear_b = [True] * nb if tracks else [rng.random() < 0.6 for _ in range(nb)]
    c_a = [rng.choice([0.1, 0.2, 0.2, INF, -0.3]) for _ in range(na)]
    c_b = None if tracks else [rng.choice([0.1, 0.2, 0.2, INF, -0.3]) for _ in range(nb)]
    clearance = [[rng.choice([0.05, 0.1, 0.1, 0.3, -0.2, INF, NAN]) for _ in range(nb)] for _ in range(na)]
    return cost_a, cost_b, clear_a, clear_b, c_a, c_b, clearance


def test_the_rule_agrees_with_a_brute_force_restatement():
    rng = random.Random(20240611)
    rules = set()
    for trial in range(400):
        na, nb = rng.randint(1, 5), rng.randint(1, 5)
        t = _random_tables(rng, na, nb, tracks=trial % 3 == 0)
        if trial % 50 == 7:      # nothing comparable at all: rule -1
            t = t[:6] + ([[NAN] * nb for _ in range(na)],)
        om, pm = rng.choice([-1.0, 0.15, 0.25]), rng.choice([-1.0, 0.1, 0.2, 1.0])
        prev = rng.choice([None, (rng.randint(-1, na - 1), rng.randint(-1, nb - 1))])
        got = ref.joint_rule(*t, om, pm, prev)
        assert got == _brute(*t, om, pm, prev), (trial, t, om, pm, prev)
        rules.add(got[1])
    assert rules == {-1, 0, 1, 2}


def test_all_nan_clearances_give_no_pair():
    r = ref.joint_rule([1.0], [1.0], [True], [True], [0.5], [0.5], [[NAN]], 0.1, 0.1)
    assert r == ((-1, -1), -1, 0)


# ---- hand cases of the rule, and the mutants they catch ----
def _rule(mut, cost_a, cost_b, clear_a, clear_b, c_a, c_b, clearance, om, pm, prev=None):
    """ref.joint_rule with ONE deliberate mistake"""
    na, nb = len(cost_a), len(cost_b)
    if mut == "mask_a":
        clear_a = [True] * na
    if mut == "mask_b":
        clear_b = [True] * nb

    def feasible(i, j):
        return clear_a[i] and clear_b[j] and clearance[i][j] >= pm

    order = [(i, j) for i in range(na) for j in range(nb)]
    if mut == "column_major":
        order = [(i, j) for j in range(nb) for i in range(na)]
    m, best, nf = (-1, -1), INF, 0
    for i, j in order:
        if feasible(i, j):
            nf += 1
            if cost_a[i] + cost_b[j] < best:
                best, m = cost_a[i] + cost_b[j], (i, j)
    if m != (-1, -1):
        if prev is not None and prev[0] >= 0 and prev[1] >= 0 and feasible(*prev):
            sp = 0.9 * (cost_a[prev[0]] + cost_b[prev[1]])
            if (best > sp) if mut == "gt" else (best >= sp):
                return tuple(prev), 0, nf
        return m, 1, nf
    pick, bg = (-1, -1), -INF
    for i, j in order:
        g, part = ref.excess(c_a[i], c_b[j], clearance[i][j], om, pm)
        if mut == "clearance_alone":
            g = clearance[i][j]
        if part and g > bg:
            bg, pick = g, (i, j)
    return (pick, 2, nf) if pick != (-1, -1) else (pick, -1, nf)


ALL = [True, True]
HAND = {
    # agent 0 of A is blocked: the cheapest pair (0, 0) is not feasible
    "mask_a": (([1.0, 5.0], [1.0, 2.0], [False, True], ALL, [0.0, 0.5], [0.5, 0.5], [[1.0, 1.0], [1.0, 1.0]], 0.1, 0.1, None),
               ((1, 0), 1, 2)),
    "mask_b": (([1.0, 5.0], [1.0, 2.0], ALL, [False, True], [0.5, 0.5], [0.0, 0.5], [[1.0, 1.0], [1.0, 1.0]], 0.1, 0.1, None),
               ((0, 1), 1, 2)),
    # S(m) = 9.0 == 0.9 * S(prev) = 0.9 * 10.0: the previous pair is kept
    "edge": (([10.0, 9.0], [0.0, 0.0], ALL, ALL, [0.5, 0.5], [0.5, 0.5], [[1.0, 1.0], [1.0, 1.0]], 0.1, 0.1, (0, 1)),
             ((0, 1), 0, 4)),
    # nobody feasible: pair (0, 0) has the greatest pair clearance but agent 0 of A is deep in an obstacle
    "fallback": (([1.0, 1.0], [1.0, 1.0], [False, False], ALL, [-0.9, 0.0], [0.5, 0.5], [[0.9, 0.2], [0.3, 0.25]], 0.1, 0.1, None),
                 ((1, 0), 2, 0)),
    # S ties at (0, 1) and (1, 0): row-major order finds (0, 1) first
    "tie": (([1.0, 2.0], [1.0, 2.0], ALL, ALL, [0.5, 0.5], [0.5, 0.5], [[-1.0, 1.0], [1.0, -1.0]], 0.1, 0.1, None),
            ((0, 1), 1, 2)),
    # ... and so does the fallback on a tie of g
    "tie_g": (([1.0, 2.0], [1.0, 2.0], ALL, ALL, [0.5, 0.5], [0.5, 0.5], [[-1.0, 0.0], [0.0, -1.0]], 0.1, 0.1, None),
              ((0, 1), 2, 0)),
    # a NaN sum of the previous pair fails the comparison: it is not kept
    "nan_prev": (([NAN, 9.0], [0.0, 0.0], ALL, ALL, [0.5, 0.5], [0.5, 0.5], [[1.0, 1.0], [1.0, 1.0]], 0.1, 0.1, (0, 0)),
                 ((1, 0), 1, 4)),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_rule_on_hand_made_tables(name):
    args, want = HAND[name]
    assert ref.joint_rule(*args) == want
    assert _rule(None, *args) == want


@pytest.mark.parametrize("mut,case", [("mask_a", "mask_a"), ("mask_b", "mask_b"), ("gt", "edge"),
                                      ("clearance_alone", "fallback"), ("column_major", "tie"), ("column_major", "tie_g")])
def test_mutants_of_the_rule_are_caught(mut, case):
    args, want = HAND[case]
    assert _rule(mut, *args) != want


# ---- the composition: window and trailing obstacle, on the hand-derived geometry of tests/test_path_audit.py ----
# two agents per side at rest; side A at the origin, side B at (1, 0, 0): every d2 is 1, the pair clearance 1 - 0.25
REST_A = [[(0.0, 0.0, 0.0)] * 7] * 2
MOVING = [1.0, 0.0, 0.0, -0.5, 0.0, 0.0, 0.25]          # c(k) = 0.625 - 0.0625 k for an agent at the origin
FAR = [9.0, 9.0, 9.0, 0.0, 0.0, 0.0, 0.25]
DT, RAD = 0.125, 0.125


def _rest(horizon, skip, lists, om=0.45, pm=0.5, paths_b=None, n=(7, 7), right_assoc=0):
    paths = [REST_A, paths_b or [[(1.0, 0.0, 0.0)] * 7] * 2]
    n_points = [[n[0]] * 2, [n[1]] * 2]
    return ref.select_pair_clear(paths, n_points, lists, [[1.0, 2.0], [1.0, 2.0]], DT, RAD, 0, 1, om, horizon, skip, 0.25, pm,
                                 None, None, right_assoc)


@pytest.mark.parametrize("right_assoc", [0, 1])
def test_hand_derived_composition(right_assoc):
    lists = [[FAR, MOVING], [FAR, FAR]]
    # the moving sphere is the TRAILING obstacle of arm 0: audited, it violates 0.45 at step 3
    r = _rest(4, 0, lists, right_assoc=right_assoc)
    assert (r["rule"], r["n_feasible"], r["n_clear"], r["first_violation"]) == (2, 0, (0, 2), (3, 4))
    assert r["obstacle_clearance"][0] == 0.4375 and r["worst_excess"] == 0.4375 - 0.45 and r["clearance"] == 0.75
    # skipped, every agent is clear and the pair is the cheapest
    r = _rest(4, 1, lists, right_assoc=right_assoc)
    assert (r["pair"], r["rule"], r["n_feasible"], r["n_clear"], r["cost"]) == ((0, 0), 1, 4, (2, 2), 2.0)
    # mutant "the trailing obstacle not skipped" is the first call: its answer differs
    assert _rest(4, 0, lists)["rule"] != r["rule"]
    # one obstacle per list and skip_trailing: nothing to audit, c = +inf
    r = _rest(4, 1, [[MOVING], [MOVING]], right_assoc=right_assoc)
    assert r["obstacle_clearance"] == (INF, INF) and r["n_clear"] == (2, 2) and r["worst_excess"] == 0.25


def test_the_window_applies_to_the_cross_audit():
    """side B walks towards side A from step 4 on: inside a window of 4 the pair keeps 0.75, over the whole path it
    does not. A mutant that audits the uncut paths reports the second answer for the first call."""
    walk = [(1.0, 0.0, 0.0)] * 4 + [(0.5, 0.0, 0.0), (0.25, 0.0, 0.0), (0.25, 0.0, 0.0)]
    lists = [[FAR, FAR], [FAR, FAR]]
    r4 = _rest(4, 0, lists, paths_b=[walk, walk])
    r7 = _rest(7, 0, lists, paths_b=[walk, walk])
    assert (r4["rule"], r4["clearance"], r4["steps"]) == (1, 0.75, (0, 0))
    assert (r7["rule"], r7["clearance"], r7["steps"]) == (2, 0.0, (5, 5))
    # the hold rule holds only what ended inside the window: side A ends after 2 points and is held at its last one
    r = _rest(7, 0, lists, paths_b=[walk, walk], n=(2, 7))
    assert (r["clearance"], r["steps"]) == (0.0, (5, 5))


# ---- the GPU shapes' parametrisation on the oracle's rollouts ----
def _oracle_tables(oracle, scenes, shape):
    P, N, M, H, ragged, _ = shape
    scs = pc.build_scenes(scenes, P, N, M, H, ragged)
    paths, n, costs = [], [], []
    for sc in scs:
        o = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
        try:
            o.set_initial_position(sc["start"])
            o.rollout()
            o.evaluate(sc["cost_gains"], sc["ws_limits"])
            pp, nn = o.paths()
            paths.append(np.asarray(pp).reshape(N, -1, 3).tolist())
            n.append(np.asarray(nn).reshape(N).tolist())
            costs.append(np.asarray(o.costs()).reshape(N).tolist())
        finally:
            o.close()
    live = pc.live_list(scenes, np.stack([s["obstacles"] for s in scs])).tolist()
    return scs, paths, n, costs, live


def run_calls(shape, tables, right_assoc):
    """the reference's answer to every call of pc.calls(shape), the audits and matrices computed once and shared"""
    scs, paths, n, costs, live = tables
    a, b = shape[5]
    aud, mat, out = {}, {}, []
    for c in pc.calls(shape):
        ka = (c["obstacle_margin"], c["horizon"], c["skip_trailing"])
        km = (c["horizon"], c["late"])
        if ka not in aud:
            aud[ka] = ref.obstacle_side(paths, n, live, scs[0]["dt"], pc.RADIUS, c["obstacle_margin"], c["horizon"],
                                        c["skip_trailing"], right_assoc)
        if km not in mat:
            mat[km] = ref.pair_side(paths[a], n[a], paths[b], n[b], c["horizon"], pc.SEP, c["late"], right_assoc)
        out.append(ref.select_pair_clear(paths, n, live, costs, scs[0]["dt"], pc.RADIUS, a, b, c["obstacle_margin"], c["horizon"],
                                         c["skip_trailing"], pc.SEP, c["pair_margin"], c["late"], c["prev_pair"], right_assoc,
                                         aud[ka], mat[km]))
    return out


def test_the_parametrisation_reaches_every_rule_and_regime(oracle, scenes):
    order = oracle.eval_order()
    rules, regimes, joint_only = set(), set(), []
    for shape in pc.SHAPES:
        tables = _oracle_tables(oracle, scenes, shape)
        scs, paths, n, costs, live = tables
        N, (a, b) = shape[1], shape[5]
        if shape[4]:
            assert len(set(n[a])) > 1 and len(set(n[b])) > 1, "the ragged case is meant to have paths of different lengths"
        full = car.cross_audit(paths[a], n[a], paths[b], n[b], pc.SEP, order)[0]
        seen = set()
        for c, r in zip(pc.calls(shape), run_calls(shape, tables, order)):
            regime = 0 if r["n_feasible"] == 0 else (2 if r["n_feasible"] == N * N else 1)
            seen.add((r["rule"], regime))
            if c["late"] is None and c["prev_pair"] is None and r["rule"] == 1:
                alone = scr.select_clear(paths, n, live, costs, scs[0]["dt"], pc.RADIUS, c["obstacle_margin"], c["horizon"], order)
                apart = car.select_pair(full, costs[a], costs[b], c["pair_margin"])[0]
                if r["pair"] != apart and r["pair"] != (alone["pick"][a], alone["pick"][b]):
                    joint_only.append((pc.shape_id(shape), c, r["pair"], apart, (alone["pick"][a], alone["pick"][b])))
        print(pc.shape_id(shape), len(pc.calls(shape)), "calls; (rule, n_feasible regime) seen:", sorted(seen))
        rules |= {r for r, _ in seen}
        regimes |= {g for _, g in seen}
    print("calls whose pair is neither select_pair's nor select_clear's two picks:", len(joint_only), joint_only[:3])
    assert rules == {0, 1, 2}
    assert regimes == {0, 1, 2}          # no pair feasible, some, all N_a * N_b
    assert joint_only, "no call of the parametrisation needs the joint rule"


# ---- the binding table, the header, the resource record and the facade ----
def test_binding_table_lists_the_exports(pmaf):
    assert {"pmaf_select_pair_clear", "pmaf_select_clear_tracks"} <= set(pmaf.planner.SYMBOLS)
    for m in ("select_pair_clear", "select_clear_tracks"):
        assert callable(getattr(pmaf.PmafPlanner, m))


def test_header_keeps_abi_7_and_declares_the_exports():
    hdr = open(os.path.join(ROOT, "include", "pmaf.h")).read()
    assert "#define PMAF_ABI_VERSION 7" in hdr
    for name in ("pmaf_select_pair_clear", "pmaf_select_clear_tracks"):
        assert "int %s(pmaf_planner *h" % name in hdr


def test_resource_record_new_kernels_use_no_scratch(pmaf, hip_lib):
    rec = os.path.join(os.path.dirname(pmaf.LIB_PATH), "resource_usage.txt")
    assert os.path.exists(rec), "csrc/build.sh keeps the record next to the library"
    scratch, name = {}, None
    for line in open(rec):
        line = line.strip()
        if line.startswith("Function Name:"):
            name = line.split(":", 1)[1].strip()
        elif name and line.startswith("ScratchSize"):
            scratch[name] = int(line.rsplit(":", 1)[1])
    for k in ("k_pairclear_window", "k_pairclear_reduce", "k_pairclear_final", "k_select_audit"):
        hits = [n for n in scratch if k in n]
        assert len(hits) == 1, (k, sorted(scratch))
        assert scratch[hits[0]] == 0, (hits[0], scratch[hits[0]])


CALLER = r'''
#include "bimanual_planning_ros/cf_manager.h"
using namespace ghostplanner::cfplanner;
int joint(CfManager &m, CfManager &other, const std::vector<Obstacle> &obstacles) {
  const std::vector<std::vector<Vector3d>> paths = {other.getSelectedPath()};
  const JointSelection a = m.selectClearAgainst(obstacles, 0.05, 50, paths, 0.15, 0.02, true);
  const JointSelection b = m.selectClearAgainst(obstacles, 0.05, 50, paths, 0.15, 0.02, 2, 0, false);
  return a.pick + a.track + a.rule + a.n_feasible + a.n_clear + a.first_violation + a.step + a.other_step +
         (a.cost + a.clearance + a.obstacle_clearance + a.worst_excess > 0.0) + b.pick;
}
'''


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_method_compiles(eigen):
    chk = os.path.join(ROOT, "tests", "cpp", "eigen_api_check")
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")]
    if eigen:
        cmd += ["-DPMAF_USE_EIGEN", "-I" + chk, "-I" + os.path.join(chk, "eigen3")]
    r = subprocess.run(cmd + ["-x", "c++", "-"], input=CALLER.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
