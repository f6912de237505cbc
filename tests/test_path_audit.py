"""Path audit (pmaf_evaluate_paths / CfManager::evaluatePath), the parts that need no GPU: the reference the GPU suite
compares with (tests/path_audit_reference.py) against answers derived by hand, its tie and NaN rules, and the C++ facade's
two methods through a compiler."""
import math
import os
import subprocess

import pytest

import conftest
import path_audit_reference as ref

ROOT = conftest.ROOT
INF = float("inf")

# An agent at rest at the origin (7 identical path points), dt = 0.125, agent radius 0.125.
# Obstacle 0 starts at (1, 0, 0) with v = (-0.5, 0, 0), radius 0.25: every track point 1 - 0.0625 k is exact, so
#   c(k, 0) = (1 - 0.0625 k) - (0.125 + 0.25) = 0.625 - 0.0625 k   exactly.
# Obstacle 1 rests at (0, 2, 0), radius 0.5: c(k, 1) = 2 - 0.625 = 1.375.
REST_PATH = [(0.0, 0.0, 0.0)] * 7
MOVING = [1.0, 0.0, 0.0, -0.5, 0.0, 0.0, 0.25]
RESTING = [0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.5]
DT, RAD = 0.125, 0.125


@pytest.mark.parametrize("right_assoc", [0, 1])
def test_hand_derived_moving_obstacle(right_assoc):
    track = ref.obstacle_track([MOVING], DT, 7)
    assert [t[0] for t in track] == [(1.0, 0.0, 0.0), (0.9375, 0.0, 0.0), (0.875, 0.0, 0.0), (0.8125, 0.0, 0.0),
                                     (0.75, 0.0, 0.0), (0.6875, 0.0, 0.0), (0.625, 0.0, 0.0)]
    c, step, obs, fv, po = ref.audit_path(REST_PATH, [MOVING], DT, RAD, 0.0, right_assoc)
    assert (c, step, obs, fv, po) == (0.25, 6, 0, 7, [0.25])
    # margins: c = 0.625, 0.5625, 0.5, 0.4375, 0.375, 0.3125, 0.25 -- strict `<`
    assert ref.audit_path(REST_PATH, [MOVING], DT, RAD, 0.45, right_assoc)[3] == 3
    assert ref.audit_path(REST_PATH, [MOVING], DT, RAD, 0.4375, right_assoc)[3] == 4
    assert ref.audit_path(REST_PATH, [MOVING], DT, RAD, 0.25, right_assoc)[3] == 7
    assert ref.audit_path(REST_PATH, [MOVING], DT, RAD, 1.0, right_assoc)[3] == 0
    # with the resting obstacle in front of it in the list
    c, step, obs, fv, po = ref.audit_path(REST_PATH, [RESTING, MOVING], DT, RAD, 0.3, right_assoc)
    assert (c, step, obs, fv, po) == (0.25, 6, 1, 6, [1.375, 0.25])
    # a shorter path sees less of the approach
    assert ref.audit_path(REST_PATH[:3], [MOVING], DT, RAD, 0.0, right_assoc)[:3] == (0.5, 2, 0)


def test_track_is_iterated_not_multiplied():
    # ten steps of 0.1 sum to 0.9999999999999999 in double, 10 * 0.1 is 1.0: the contract is the iterated sum
    # (CfAgent::predictObstacles)
    tr = ref.obstacle_track([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.1]], 0.1, 11)
    assert tr[10][0][0] == 0.9999999999999999 and 10 * 0.1 == 1.0
    assert tr[6][0][0] == 0.6 and 6 * 0.1 == 0.6000000000000001


def test_dot_association_is_the_callers():
    # d = (1.5 * 2^26, 1, 1): the squares 9 * 2^50 (ulp 2), 1, 1 are exact. Left-associated, each 1 is half an ulp and
    # ties to the even 9 * 2^50 twice; right-associated, 1 + 1 = 2 is one ulp and survives
    x0 = 1.5 * 2.0 ** 26
    x = (x0, 1.0, 1.0)
    left = ref.clearance_pair(x, (0.0, 0.0, 0.0), 0.0, 0)
    right = ref.clearance_pair(x, (0.0, 0.0, 0.0), 0.0, 1)
    assert left == x0
    assert right == math.sqrt(x0 * x0 + 2.0) == x0 + 2.0 ** -26


def test_ties_go_to_the_smallest_step_then_the_smallest_obstacle():
    twin = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.25]
    far = [0.0, 9.0, 0.0, 0.0, 0.0, 0.0, 0.25]
    # identical obstacles at indices 1 and 2, identical path points: the first pair in (k, j) order wins
    c, step, obs, fv, po = ref.audit_path(REST_PATH, [far, twin, twin], DT, RAD, 0.7, 0)
    assert (c, step, obs, fv) == (0.625, 0, 1, 0) and po == [8.625, 0.625, 0.625]
    # a margin at the clearance is not violated (strict)
    assert ref.audit_path(REST_PATH, [far, twin, twin], DT, RAD, 0.625, 0)[3] == 7
    # an obstacle that ties LATER in k with a smaller index does not take over: k decides before j.
    # obstacle 0 reaches y = 1 at step 4 (1.5 - 4 * 0.125), obstacle 1 rests there from step 0 on
    comer = [0.0, 1.5, 0.0, 0.0, -1.0, 0.0, 0.25]
    c, step, obs, _, po = ref.audit_path(REST_PATH[:5], [comer, twin], DT, RAD, 0.0, 0)
    assert (c, step, obs) == (0.625, 0, 1) and po == [0.625, 0.625]


def test_nan_never_wins_and_empty_paths():
    nan = float("nan")
    path = [(nan, 0.0, 0.0), (0.0, 0.0, 0.0)]
    c, step, obs, fv, po = ref.audit_path(path, [RESTING], DT, RAD, 2.0, 0)
    assert (c, step, obs, fv, po) == (1.375, 1, 0, 1, [1.375])
    c, step, obs, fv, po = ref.audit_path(path[:1], [RESTING], DT, RAD, 2.0, 0)
    assert (c, step, obs, fv, po) == (INF, -1, -1, 1, [INF])
    assert ref.audit_path([], [RESTING], DT, RAD, 2.0, 0) == (INF, -1, -1, 0, [INF])


def test_audit_over_populations_shares_one_track():
    paths = [[REST_PATH, REST_PATH[:3] + [(9.0, 9.0, 9.0)] * 4]]
    r = ref.audit(paths, [[7, 3]], [[RESTING, MOVING]], DT, RAD, 0.3, 0)
    assert r["clearance"] == [[0.25, 0.5]] and r["step"] == [[6, 2]] and r["obstacle"] == [[1, 1]]
    assert r["first_violation"] == [[6, 3]] and r["per_obstacle"] == [[[1.375, 0.25], [1.375, 0.5]]]


def test_binding_table_lists_the_audit_exports(pmaf):
    assert {"pmaf_evaluate_paths", "pmaf_evaluate_path"} <= set(pmaf.planner.SYMBOLS)
    assert callable(pmaf.PmafPlanner.evaluate_paths) and callable(pmaf.PmafPlanner.evaluate_path)


CALLER = r'''
#include "bimanual_planning_ros/cf_manager.h"
using namespace ghostplanner::cfplanner;
// the reference's declaration (B/include/bimanual_planning_ros/cf_manager.h:130), as a member pointer
double (CfManager::*const kEvaluatePath)(const std::vector<Obstacle> &) = &CfManager::evaluatePath;
double audit(CfManager &m, const std::vector<Obstacle> &obstacles, std::vector<int> &unsafe_from) {
  const double selected = m.evaluatePath(obstacles);
  const PathAudit all = m.evaluatePaths(obstacles, 0.02);
  const PathAudit dflt = m.evaluatePaths(obstacles);
  unsafe_from = all.first_violation;
  double least = selected;
  for (size_t a = 0; a < all.clearance.size(); ++a)
    if (all.clearance[a] < least && all.step[a] >= 0 && all.obstacle[a] >= 0) least = all.clearance[a];
  return least + dflt.clearance.at(0);
}
'''


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_evaluate_path_compiles(eigen):
    """CfManager::evaluatePath with the reference's signature and evaluatePaths through a compiler: plain build and the
    PMAF_USE_EIGEN branch against the declaration-only Eigen header (tests/cpp/eigen_api_check), the way
    test_facade.py::test_eigen_branch_api_shape builds its units"""
    chk = os.path.join(ROOT, "tests", "cpp", "eigen_api_check")
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")]
    if eigen:
        cmd += ["-DPMAF_USE_EIGEN", "-I" + chk, "-I" + os.path.join(chk, "eigen3")]
    r = subprocess.run(cmd + ["-x", "c++", "-"], input=CALLER.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
