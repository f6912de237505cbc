"""Selection against the live list (pmaf_select_clear / pmaf_adopt_best), the parts that need no GPU: the reference the
GPU suite compares with (tests/select_clear_reference.py) on hand-made tables, properties over random tables, nine
mutants of the rule that the hand cases must catch, the binding table and the C++ facade through a compiler."""
import os
import random
import subprocess

import pytest

import conftest
import path_audit_reference as par
import select_clear_reference as ref

ROOT = conftest.ROOT
INF = float("inf")
NAN = float("nan")


# ---- the rule on hand-made tables: (cost, fv, w, c, prev) -> (pick, rule, n_clear) ----
W = [5, 5, 5, 5]
C = [0.5, 0.4, 0.3, 0.2]
HAND = {
    # rule 1: agents 1 and 3 are clear, 3 is cheaper
    "rule1": (([1.0, 8.0, 2.0, 6.0], [2, 5, 3, 5], W, C, None), (3, 1, 2)),
    # rule 0: the previous pick 1 is clear and 6.0 >= 0.9 * 6.5
    "rule0": (([1.0, 6.5, 2.0, 6.0], [2, 5, 3, 5], W, C, 1), (1, 0, 2)),
    # ... and loses it when the cheapest clear agent is more than 10 % cheaper: 5.0 < 0.9 * 6.5
    "rule0_lost": (([1.0, 6.5, 2.0, 5.0], [2, 5, 3, 5], W, C, 1), (3, 1, 2)),
    # rule 2: nobody is clear; agent 2 stays clear longest
    "rule2": (([1.0, 2.0, 3.0, 4.0], [2, 1, 4, 3], W, C, 0), (2, 2, 0)),
    # a tie on cost goes to the smallest index
    "tie": (([7.0, 3.0, 3.0, 3.0], [5, 5, 5, 5], W, C, None), (1, 1, 4)),
    # cost[m] == 0.9 * cost[q] keeps q (9.0 == 0.9 * 10.0 in double)
    "edge": (([10.0, 9.0, 20.0, 20.0], [5, 5, 5, 5], W, C, 0), (0, 0, 4)),
    # a NaN previous cost is dropped (the reference's !(a < b) would keep it)
    "nan_prev": (([NAN, 9.0, 20.0, 20.0], [5, 5, 5, 5], W, C, 0), (1, 1, 4)),
    # NaN and +infinite costs never win
    "nan_inf": (([NAN, INF, 4.0, NAN], [5, 5, 5, 5], W, C, None), (2, 1, 4)),
    # all costs NaN: no comparable cost, rule 2 (every agent clear: fv ties, the greatest c, agent 0)
    "all_nan": (([NAN, NAN, NAN, NAN], [5, 5, 5, 5], W, C, 2), (0, 2, 4)),
    # the only clear agent costs +infinity: it does not win, rule 2 picks it as the agent that stays clear longest
    "inf_only": (([1.0, INF, 2.0, 3.0], [2, 5, 3, 4], W, C, None), (1, 2, 1)),
    # the fallback order: fv first (agent 1 and 3 tie at 4), then c (0.4 > 0.2), then the index
    "fallback_c": (([1.0, 2.0, 3.0, 4.0], [2, 4, 3, 4], W, [0.5, 0.2, 0.3, 0.4], None), (3, 2, 0)),
    "fallback_idx": (([1.0, 2.0, 3.0, 4.0], [2, 4, 3, 4], W, [0.5, 0.2, 0.3, 0.2], None), (1, 2, 0)),
    # ... and a greater clearance does not beat a later first violation
    "fallback_fv": (([1.0, 2.0, 3.0, 4.0], [1, 2, 4, 3], W, [0.9, 0.8, 0.1, 0.7], None), (2, 2, 0)),
    # w = 0 counts as clear (fv = 0 == w): the empty path is the only clear one
    "w0": (([5.0, 1.0, 9.0, 1.0], [2, 0, 0, 3], [5, 5, 0, 5], [0.1, 0.1, INF, 0.1], None), (2, 1, 1)),
    # the previous pick is blocked: not kept although its cost would keep it
    "prev_blocked": (([1.0, 6.5, 2.0, 6.4], [2, 3, 3, 5], W, C, 1), (3, 1, 1)),
    # fv equals the window, not the path length: paths of 7 points under horizon 3
    "window": (([1.0, 2.0, 3.0, 4.0], [3, 1, 3, 2], [3, 3, 3, 3], C, None), (0, 1, 2)),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_rule_on_hand_made_tables(name):
    args, want = HAND[name]
    assert ref.pick(*args) == want


def test_prev_minus_one_and_none_behave_alike():
    for name, (args, want) in HAND.items():
        cost, fv, w, c, _ = args
        assert ref.pick(cost, fv, w, c, -1) == ref.pick(cost, fv, w, c, None), name
    assert ref.pick([1.0, 6.5, 2.0, 6.0], [2, 5, 3, 5], W, C, -1) == (3, 1, 2)


# ---- the window audit on the hand-derived geometry of tests/test_path_audit.py: c(k) = 0.625 - 0.0625 k ----
REST_PATH = [(0.0, 0.0, 0.0)] * 7
MOVING = [1.0, 0.0, 0.0, -0.5, 0.0, 0.0, 0.25]
DT, RAD = 0.125, 0.125


def _rest_select(margin, horizon, right_assoc=0, n=7):
    return ref.select_clear([[REST_PATH]], [[n]], [[MOVING]], [[1.0]], DT, RAD, margin, horizon, right_assoc)


@pytest.mark.parametrize("right_assoc", [0, 1])
def test_hand_derived_window(right_assoc):
    # c = 0.625, 0.5625, 0.5, 0.4375, ...: margin 0.45 is first violated at step 3
    r = _rest_select(0.45, 3, right_assoc)
    assert (r["pick"], r["rule"], r["n_clear"], r["clearance"], r["first_violation"]) == ([0], [1], [1], [0.5], [3])
    r = _rest_select(0.45, 4, right_assoc)
    assert (r["pick"], r["rule"], r["n_clear"], r["clearance"], r["first_violation"]) == ([0], [2], [0], [0.4375], [3])
    # a horizon past the path: the whole path, fv = n when clear
    r = _rest_select(0.2, 100, right_assoc)
    assert (r["rule"], r["clearance"], r["first_violation"]) == ([1], [0.25], [7])
    # an empty path is clear with +infinity
    r = _rest_select(10.0, 4, right_assoc, n=0)
    assert (r["rule"], r["n_clear"], r["clearance"], r["first_violation"]) == ([1], [1], [INF], [0])


# ---- properties over random tables ----
def _random_scene(rng, P=2, N=5, cap=9, n_obs=3):
    paths = [[[(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1)) for _ in range(cap)] for _ in range(N)]
             for _ in range(P)]
    n_points = [[rng.randint(0, cap) for _ in range(N)] for _ in range(P)]
    obstacles = [[[rng.uniform(-1, 1) for _ in range(3)] + [rng.uniform(-0.5, 0.5) for _ in range(3)] + [rng.uniform(0.05, 0.3)]
                  for _ in range(n_obs)] for _ in range(P)]
    costs = [[rng.choice([rng.uniform(1, 10), rng.uniform(1, 10), 3.0, INF, NAN]) for _ in range(N)] for _ in range(P)]
    return paths, n_points, obstacles, costs


def test_properties_over_random_tables():
    rng = random.Random(20240607)
    rules = set()
    for trial in range(60):
        cap = 9
        paths, n_points, obstacles, costs = _random_scene(rng, cap=cap)
        horizon = rng.randint(1, cap + 2)
        prev = rng.choice([None, [rng.randint(-1, 4) for _ in range(2)]])
        last = None
        for margin in (-2.0, 0.0, 0.1, 0.3, 0.6, 1.0, 4.0):
            r = ref.select_clear(paths, n_points, obstacles, costs, 0.1, 0.05, margin, horizon, trial & 1, prev)
            assert all(0 <= i < 5 for i in r["pick"])                     # the pick is always in range
            if last is not None:
                assert all(a <= b for a, b in zip(r["n_clear"], last))    # n_clear never grows with the margin
            last = r["n_clear"]
            rules.update(r["rule"])
        # at horizon = cap the window audit equals audit() on the full paths
        c, fv, w = ref.window_audit(paths, n_points, obstacles, 0.1, 0.05, 0.3, cap, trial & 1)
        full = par.audit(paths, n_points, obstacles, 0.1, 0.05, 0.3, trial & 1)
        assert w == [[int(n) for n in row] for row in n_points]
        assert repr(c) == repr(full["clearance"]) and fv == full["first_violation"]
    assert rules == {0, 1, 2}


# ---- nine mutants of the rule, each caught by at least one hand case ----
def _mutant_pick(mut, cost, fv, w, c, prev=None, n=None):
    """ref.pick with ONE deliberate mistake; n = the path lengths (mutant 'fv_vs_n')"""
    N = len(cost)
    if mut == "fv_vs_n":
        clear = [fv[a] == n[a] for a in range(N)]
    else:
        clear = [fv[a] == w[a] for a in range(N)]
    n_clear = sum(clear)
    m, best = -1, INF
    for a in range(N):
        if not clear[a]:
            continue
        if mut == "le":
            better = cost[a] <= best
        elif mut == "last_tie":
            better = cost[a] < best or (cost[a] == best and cost[a] < INF)
        elif mut == "inf_wins":
            better = cost[a] < best or (m < 0 and cost[a] == INF)
        else:
            better = cost[a] < best
        if better:
            best, m = cost[a], a
    if m >= 0:
        if prev is not None and int(prev) >= 0:
            q = int(prev)
            if mut == "other_side":
                keep = 0.9 * cost[m] >= cost[q]
            elif mut == "not_less":
                keep = not (cost[m] < 0.9 * cost[q])
            else:
                keep = cost[m] >= 0.9 * cost[q]
            if (clear[q] or mut == "prev_blocked") and keep:
                return q, 0, n_clear
        return m, 1, n_clear
    p = 0
    for a in range(1, N):
        if mut == "clearance_first":
            if c[a] > c[p] or (c[a] == c[p] and fv[a] > fv[p]):
                p = a
        elif fv[a] > fv[p] or (fv[a] == fv[p] and c[a] > c[p]):
            p = a
    return p, 2, n_clear


def _caught_by(mut, names):
    """the hand cases among `names` on which the mutant's answer differs from the literal expectation"""
    out = []
    for name in names:
        (cost, fv, w, c, prev), want = HAND[name]
        if _mutant_pick(mut, cost, fv, w, c, prev, n=[7] * len(cost)) != want:
            out.append(name)
    return out


def test_the_unmutated_copy_passes_every_hand_case():
    assert _caught_by(None, sorted(HAND)) == []


def test_mutant_le_for_less_is_caught():
    assert "tie" in _caught_by("le", ["tie"])


def test_mutant_factor_on_the_other_side_is_caught():
    assert "rule0" in _caught_by("other_side", ["rule0"])


def test_mutant_not_less_for_greater_equal_is_caught():
    assert "nan_prev" in _caught_by("not_less", ["nan_prev"])


def test_mutant_last_index_on_ties_is_caught():
    assert "tie" in _caught_by("last_tie", ["tie"])


def test_mutant_prev_kept_although_blocked_is_caught():
    assert "prev_blocked" in _caught_by("prev_blocked", ["prev_blocked"])


def test_mutant_fallback_by_clearance_first_is_caught():
    assert "fallback_fv" in _caught_by("clearance_first", ["fallback_fv"])


def test_mutant_window_plus_one_is_caught():
    # the window audit with w + 1 points sees step 3 of the hand-derived geometry: blocked where the contract says clear
    want = _rest_select(0.45, 3)
    got = _rest_select(0.45, 3 + 1)
    assert (want["rule"], want["n_clear"]) == ([1], [1])
    assert (got["rule"], got["n_clear"]) != (want["rule"], want["n_clear"])


def test_mutant_fv_compared_with_n_is_caught():
    assert "window" in _caught_by("fv_vs_n", ["window"])


def test_mutant_infinity_allowed_to_win_is_caught():
    assert "inf_only" in _caught_by("inf_wins", ["inf_only"])


# ---- the binding table and the facade ----
def test_binding_table_lists_the_exports(pmaf):
    assert {"pmaf_select_clear", "pmaf_adopt_best"} <= set(pmaf.planner.SYMBOLS)
    for m in ("select_clear", "adopt_best", "audited_tick"):
        assert callable(getattr(pmaf.PmafPlanner, m))


def test_header_keeps_abi_7_and_declares_the_exports():
    hdr = open(os.path.join(ROOT, "include", "pmaf.h")).read()
    assert "#define PMAF_ABI_VERSION 7" in hdr
    for name in ("pmaf_select_clear", "pmaf_adopt_best"):
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
    for k in ("k_select_stage", "k_select_audit", "k_select_pick", "k_adopt_best"):
        hits = [n for n in scratch if k in n]
        assert len(hits) == 1, (k, sorted(scratch))
        assert scratch[hits[0]] == 0, (hits[0], scratch[hits[0]])


CALLER = r'''
#include "bimanual_planning_ros/cf_manager.h"
using namespace ghostplanner::cfplanner;
int audited(CfManager &m, const std::vector<Obstacle> &obstacles, const Vector6d &limits, ClearSelection &out) {
  const ClearSelection a = m.selectClear(obstacles, 0.05, 50);
  const ClearSelection b = m.selectClear(obstacles, 0.05, 50, false);
  m.adoptBest(b.pick);
  Vector3d next;
  const int pick = m.planTickAudited(obstacles, 0.01, 1.0, 1.0, 1.0, 1.0, limits, 0.05, 50, &next, &out);
  const int again = m.planTickAudited(obstacles, 0.01, 1.0, 1.0, 1.0, 1.0, limits, 0.05, 50);
  return a.pick + a.rule + a.n_clear + a.first_violation + (a.cost + a.clearance > 0.0) + pick + again;
}
'''


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_methods_compile(eigen):
    chk = os.path.join(ROOT, "tests", "cpp", "eigen_api_check")
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")]
    if eigen:
        cmd += ["-DPMAF_USE_EIGEN", "-I" + chk, "-I" + os.path.join(chk, "eigen3")]
    r = subprocess.run(cmd + ["-x", "c++", "-"], input=CALLER.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
