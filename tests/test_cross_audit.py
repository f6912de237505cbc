"""Cross audit (pmaf_cross_audit / pmaf_cross_audit_tracks / pmaf_select_pair), the parts that need no GPU: the
reference the GPU suite compares with (tests/cross_audit_reference.py) against answers derived by hand, the pair rule on
small literal matrices, the symmetry of the audit on oracle-made dual-arm paths, and the C++ facade's new member through
a compiler."""
import math
import os
import subprocess

import numpy as np
import pytest

import conftest
import cross_audit_reference as ref

ROOT = conftest.ROOT
INF = float("inf")
NAN = float("nan")


@pytest.mark.parametrize("right_assoc", [0, 1])
def test_hand_derived_pairs(right_assoc):
    # two one-point paths, offset (0.375, 0.5, 0): d2 = 0.140625 + 0.25 = 0.390625 exactly, root 0.625
    assert ref.pair_clearance([(0.0, 0.0, 0.0)], [(0.375, 0.5, 0.0)], 0.125, right_assoc) == (0.5, 0)
    assert ref.pair_clearance([(0.375, 0.5, 0.0)], [(0.0, 0.0, 0.0)], 1.0, right_assoc) == (-0.375, 0)   # no floor
    # a short path HELD at (0, 0, 0) against a longer one that walks along x through it: x = 1, 0.75, .., 0, .., -0.5
    walker = [(0.25 * (4 - k), 0.0, 0.0) for k in range(7)]
    assert ref.pair_clearance([(0.0, 0.0, 0.0)] * 2, walker, 0.125, right_assoc) == (-0.125, 4)
    # ... and the walker ending early: held at x = 0.5 from step 2 on, K = max(n, m) = 5, the tie goes to step 2
    assert ref.pair_clearance([(0.0, 0.0, 0.0)] * 5, walker[:3], 0.125, right_assoc) == (0.375, 2)
    # without the hold the short path would have seen only steps 0 and 1
    assert ref.pair_clearance(walker, [(0.0, 3.0, 4.0)], 0.0, right_assoc) == (5.0, 4)
    # all distances equal: step 0
    assert ref.pair_clearance([(0.0, 0.0, 0.0)] * 7, [(0.375, 0.5, 0.0)] * 4, 0.125, right_assoc) == (0.5, 0)
    # empty paths
    assert ref.pair_clearance([], walker, 0.125, right_assoc) == (INF, -1)
    assert ref.pair_clearance(walker, [], 0.125, right_assoc) == (INF, -1)


def test_nan_never_wins():
    a = [(0.0, 0.0, 0.0), (NAN, 0.0, 0.0), (0.0, 0.0, 0.0)]
    b = [(2.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]
    assert ref.pair_clearance(a, b, 0.5, 0) == (0.5, 2)
    # a path that turns NaN and is held there: only its finite steps can win
    assert ref.pair_clearance(a[:2], b, 0.5, 0) == (1.5, 0)
    c, s = ref.pair_clearance([(NAN, 0.0, 0.0)], b, 0.5, 0)
    assert (c, s) == (INF, -1)


def test_dot_association_is_the_callers():
    # d = (1.5 * 2^26, 1, 1): left-associated each 1 is half an ulp of 9 * 2^50 and ties to even twice; right-associated
    # 1 + 1 = 2 is one ulp and survives (tests/test_path_audit.py)
    x0 = 1.5 * 2.0 ** 26
    assert ref.squared_distance((x0, 1.0, 1.0), (0.0, 0.0, 0.0), 0) == x0 * x0
    assert ref.squared_distance((x0, 1.0, 1.0), (0.0, 0.0, 0.0), 1) == x0 * x0 + 2.0
    assert ref.pair_clearance([(x0, 1.0, 1.0)], [(0.0, 0.0, 0.0)], 0.0, 1)[0] == math.sqrt(x0 * x0 + 2.0)


def test_matrix_layout():
    a = [[(0.0, 0.0, 0.0)] * 3, [(0.0, 1.0, 0.0)] * 3]
    b = [[(3.0, 0.0, 4.0)] * 3, [(0.0, 0.0, 2.0)] * 3, [(9.0, 9.0, 9.0)] * 3]
    c, s = ref.cross_audit(a, [3, 1], b, [3, 2, 0], 1.0, 0)
    assert c == [[4.0, 1.0, INF], [math.sqrt(26.0) - 1.0, math.sqrt(5.0) - 1.0, INF]]
    assert s == [[0, 0, -1], [0, 0, -1]]


def test_pair_rule():
    cost_a, cost_b = [3.0, 1.0, 2.0], [5.0, 4.0]
    clr = [[0.3, 0.1], [0.05, 0.2], [0.2, 0.2]]
    # feasible minimum: (1, 1) has the least sum 5 and keeps 0.2 >= 0.1
    assert ref.select_pair(clr, cost_a, cost_b, 0.1) == ((1, 1), 5.0, 0.2, 1)
    # a margin AT a clearance is kept (>=); above it the pair falls out and only (0, 0) is left
    assert ref.select_pair(clr, cost_a, cost_b, 0.2) == ((1, 1), 5.0, 0.2, 1)
    assert ref.select_pair(clr, cost_a, cost_b, 0.25) == ((0, 0), 8.0, 0.3, 1)
    # ties go to the smallest i, then the smallest j: the sum 5 at (1, 0) and (2, 0); at all four pairs
    assert ref.select_pair([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]], [2.0, 1.0, 1.0], [4.0, 5.0], 0.5) == ((1, 0), 5.0, 1.0, 1)
    assert ref.select_pair([[1.0, 1.0], [1.0, 1.0]], [1.0, 1.0], [4.0, 4.0], 0.5) == ((0, 0), 5.0, 1.0, 1)
    # row-major does not mean the first row wins: 2 + 3 = 5 at (0, 0) against 1 + 3 = 4 at (1, 0)
    assert ref.select_pair([[1.0, 1.0], [1.0, 1.0]], [2.0, 1.0], [3.0, 4.0], 0.5) == ((1, 0), 4.0, 1.0, 1)
    # all infeasible: the greatest clearance, ties to the first in row-major order
    assert ref.select_pair(clr, cost_a, cost_b, 0.5) == ((0, 0), 8.0, 0.3, 0)
    assert ref.select_pair([[0.1, 0.3], [0.3, 0.2]], [1.0, 2.0], [4.0, 8.0], 0.5) == ((0, 1), 9.0, 0.3, 0)
    # +inf clearance (an empty path) is feasible
    assert ref.select_pair([[0.0, INF]], [1.0], [1.0, 2.0], 10.0) == ((0, 1), 3.0, INF, 1)


def test_pair_rule_nan():
    # a NaN cost never wins although its pair is feasible and would be cheapest
    assert ref.select_pair([[1.0, 1.0], [1.0, 1.0]], [NAN, 7.0], [1.0, 2.0], 0.5) == ((1, 0), 8.0, 1.0, 1)
    # a NaN clearance is infeasible and never the greatest
    assert ref.select_pair([[NAN, 0.2], [0.1, NAN]], [0.0, 0.0], [0.0, 9.0], 0.15) == ((0, 1), 9.0, 0.2, 1)
    assert ref.select_pair([[NAN, 0.2], [0.1, NAN]], [0.0, 0.0], [0.0, 9.0], 0.5) == ((0, 1), 9.0, 0.2, 0)
    # feasible pairs whose sums are all NaN or +inf: nothing won, fall back to the greatest clearance; its cost is reported
    pair, cost, clr, feas = ref.select_pair([[1.0, 2.0]], [NAN], [1.0, 2.0], 0.5)
    assert (pair, clr, feas) == ((0, 1), 2.0, 0) and math.isnan(cost)
    assert ref.select_pair([[1.0, 2.0]], [INF], [1.0, 2.0], 0.5) == ((0, 1), INF, 2.0, 0)
    # nothing comparable at all
    pair, cost, clr, feas = ref.select_pair([[NAN, NAN]], [1.0], [1.0, 2.0], 0.5)
    assert pair == (-1, -1) and feas == 0 and math.isnan(cost) and math.isnan(clr)
    pair, cost, clr, feas = ref.select_pair([[-INF]], [1.0], [1.0], 0.5)
    assert pair == (-1, -1) and feas == 0


def test_symmetry_on_oracle_made_dual_arm_paths(pmaf, scenes, oracle):
    """rollouts of scenes.dual_arm_scenes on the CPU oracle: the matrix of (A, B) is the transpose of (B, A) bit for bit
    (x - y and y - x differ in sign only, the squares are equal), and it is not constant"""
    arms = scenes.dual_arm_scenes(6, 40, 4)
    sets = []
    for sc in arms:
        o = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
        try:
            o.set_initial_position(sc["start"])
            o.rollout()
            p, n = o.paths()
            sets.append((np.asarray(p).tolist(), np.asarray(n).tolist()))
        finally:
            o.close()
    order = oracle.eval_order()
    ab_c, ab_s = ref.cross_audit(sets[0][0], sets[0][1], sets[1][0], sets[1][1], 0.15, order)
    ba_c, ba_s = ref.cross_audit(sets[1][0], sets[1][1], sets[0][0], sets[0][1], 0.15, order)
    ab_c, ba_c = np.asarray(ab_c), np.asarray(ba_c)
    assert (ab_c.view(np.uint64) == np.ascontiguousarray(ba_c.T).view(np.uint64)).all()
    assert ab_s == np.asarray(ba_s).T.tolist()
    assert np.isfinite(ab_c).all() and len(set(ab_c.reshape(-1).tolist())) > 1
    assert (np.asarray(ab_s) >= 0).all()


def test_binding_table_lists_the_cross_audit_exports(pmaf):
    assert {"pmaf_cross_audit", "pmaf_cross_audit_tracks", "pmaf_select_pair"} <= set(pmaf.planner.SYMBOLS)
    for m in ("cross_audit", "cross_audit_tracks", "select_pair"):
        assert callable(getattr(pmaf.PmafPlanner, m))
    assert callable(pmaf.shard.DualArmCoupling.pair_tick)


def test_library_exports_the_cross_audit_calls(hip_lib):
    for name in ("pmaf_cross_audit", "pmaf_cross_audit_tracks", "pmaf_select_pair"):
        assert getattr(hip_lib, name) is not None


CALLER = r'''
#include "bimanual_planning_ros/cf_manager.h"
using namespace ghostplanner::cfplanner;
CrossAudit (CfManager::*const kCrossAudit)(const std::vector<std::vector<Vector3d>> &, double) = &CfManager::crossAudit;
double closest(CfManager &left, CfManager &right, int &agent, int &other, int &step) {
  const CrossAudit r = left.crossAudit(right.getPredictedPaths(), 0.15);
  double least = r.at(0, 0);
  agent = other = 0;
  for (int i = 0; i < r.n_agents; ++i)
    for (int j = 0; j < r.n_other; ++j)
      if (r.at(i, j) < least) { least = r.at(i, j); agent = i; other = j; }
  step = r.step_at(agent, other);
  return least + r.clearance.at(0) + r.step.at(0);
}
'''


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_cross_audit_compiles(eigen):
    """CfManager::crossAudit through a compiler: plain build and the PMAF_USE_EIGEN branch against the declaration-only
    Eigen header (tests/cpp/eigen_api_check), the way tests/test_path_audit.py builds its unit"""
    chk = os.path.join(ROOT, "tests", "cpp", "eigen_api_check")
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")]
    if eigen:
        cmd += ["-DPMAF_USE_EIGEN", "-I" + chk, "-I" + os.path.join(chk, "eigen3")]
    r = subprocess.run(cmd + ["-x", "c++", "-"], input=CALLER.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
