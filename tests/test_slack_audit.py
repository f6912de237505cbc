"""Cross audit with timing slack (pmaf_cross_audit_slack / pmaf_cross_audit_tracks_slack / pmaf_select_pair_slack), the
parts that need no GPU: the reference the GPU suite compares with (tests/slack_audit_reference.py) against answers
derived by hand and against the properties include/pmaf.h states, the bindings, the C++ facade's overload through a
compiler, and the new kernel's line in the build's resource record."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import conftest
import cross_audit_reference as ref
import slack_audit_reference as sref

ROOT = conftest.ROOT
INF = float("inf")
NAN = float("nan")
WALKER = [(0.25 * (4 - k), 0.0, 0.0) for k in range(7)]     # x = 1, 0.75, .., 0 at step 4, .., -0.5
REST = [(0.0, 0.0, 0.0)] * 7


@pytest.mark.parametrize("right_assoc", [0, 1])
@pytest.mark.parametrize("late_b", [0, 3])
@pytest.mark.parametrize("late_a", [0, 1, 5])
def test_known_answers_at_rest(late_a, late_b, right_assoc):
    """A rests at the origin, so d2(k, l) depends on l alone and every admitted k ties.
    The walker passes through the origin at l = 4 (d2 = 0, clearance -0.125 with separation 0.125): admitted with
    4 - late_a <= k <= 4 + late_b, the tie goes to the smallest k.
    The walker that ends after 3 points is held at x = 0.5 from l = 2 on (d2 = 0.25, clearance 0.375): the smallest k
    with an admitted l >= 2 is max(0, 2 - late_a), and l = 2 is admitted for it (k <= 2)."""
    assert sref.pair_clearance_slack(REST, WALKER, 0.125, late_a, late_b, right_assoc) == (-0.125, max(0, 4 - late_a), 4)
    assert sref.pair_clearance_slack(REST, WALKER[:3], 0.125, late_a, late_b, right_assoc) == (0.375, max(0, 2 - late_a), 2)
    # the roles exchanged: the walker is A, late_b lets the resting B ... which changes nothing but the tie's l
    assert sref.pair_clearance_slack(WALKER, REST, 0.125, late_a, late_b, right_assoc) == (-0.125, 4, max(0, 4 - late_b))
    # two paths at rest, offset (0.375, 0.5, 0): every admitted pair ties at d2 = 0.390625, root 0.625
    assert sref.pair_clearance_slack(REST, [(0.375, 0.5, 0.0)] * 4, 0.125, late_a, late_b, right_assoc) == (0.5, 0, 0)
    # empty paths
    assert sref.pair_clearance_slack([], WALKER, 0.125, late_a, late_b, right_assoc) == (INF, -1, -1)
    assert sref.pair_clearance_slack(WALKER, [], 0.125, late_a, late_b, right_assoc) == (INF, -1, -1)


def test_the_slack_decides():
    """two walkers on parallel lines 0.5 apart, B three steps ahead of A's schedule: step against step they are never
    closer than sqrt(0.5^2 + 0.75^2); with A late by 3 they pass at 0.5"""
    a = [(0.25 * k, 0.0, 0.0) for k in range(8)]
    b = [(0.25 * (k - 3), 0.5, 0.0) for k in range(8)]
    assert sref.pair_clearance_slack(a, b, 0.0, 0, 0, 0) == (math.sqrt(0.25 + 0.5625), 0, 0)
    assert sref.pair_clearance_slack(a, b, 0.0, 2, 0, 0) == (math.sqrt(0.25 + 0.0625), 0, 2)
    assert sref.pair_clearance_slack(a, b, 0.0, 3, 0, 0) == (0.5, 0, 3)
    assert sref.pair_clearance_slack(a, b, 0.0, 0, 3, 0)[0] == math.sqrt(0.25 + 0.5625)      # the wrong arm's slack: no help
    # the hold rule in the window: B ends after 2 points and waits at x = -0.5; A's point 0 is the closest to it
    assert sref.pair_clearance_slack(a, b[:2], 0.0, 7, 0, 0) == (math.sqrt(0.25 + 0.25), 0, 1)


def test_nan_never_wins():
    a = [(0.0, 0.0, 0.0), (NAN, 0.0, 0.0), (0.0, 0.0, 0.0)]
    b = [(2.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]
    assert sref.pair_clearance_slack(a, b, 0.5, 0, 0, 0) == (0.5, 2, 2)
    assert sref.pair_clearance_slack(a, b, 0.5, 1, 0, 0) == (-0.5, 0, 1)      # A's point 0 against B's point 1
    assert sref.pair_clearance_slack(a, b, 0.5, 0, 1, 0) == (-0.5, 2, 1)
    assert sref.pair_clearance_slack([(NAN, 0.0, 0.0)], b, 0.5, 2, 2, 0) == (INF, -1, -1)


def _random_ragged(seed, n_a, n_b, cap):
    rng = np.random.default_rng(seed)
    pa = rng.uniform(-1.0, 1.0, (n_a, cap, 3))
    pb = rng.uniform(-1.0, 1.0, (n_b, cap, 3))
    # smooth paths (cumulative small steps), so that neighbouring steps are close and the slack matters
    pa = np.cumsum(pa * 0.05, axis=1)
    pb = np.cumsum(pb * 0.05, axis=1) + np.array([0.2, 0.0, 0.0])
    la = rng.integers(0, cap + 1, n_a)
    lb = rng.integers(0, cap + 1, n_b)
    la[0], lb[0] = cap, 1
    if n_a > 1:
        la[1] = 0
    return pa.tolist(), la.tolist(), pb.tolist(), lb.tolist()


def _bits(m):
    return np.ascontiguousarray(np.asarray(m, dtype=np.float64)).view(np.uint64)


@pytest.mark.parametrize("right_assoc", [0, 1])
def test_zero_slack_is_the_cross_audit(right_assoc):
    pa, la, pb, lb = _random_ragged(3, 5, 4, 19)
    want_c, want_s = ref.cross_audit(pa, la, pb, lb, 0.15, right_assoc)
    c, sa, sb = sref.cross_audit_slack(pa, la, pb, lb, 0.15, 0, 0, right_assoc)
    assert (_bits(c) == _bits(want_c)).all()
    assert sa == want_s and sb == want_s
    assert np.isinf(np.asarray(c)[1]).all() and (np.asarray(sa)[1] == -1).all()     # the empty path of A


def test_clearance_never_grows_with_either_slack():
    pa, la, pb, lb = _random_ragged(4, 4, 5, 17)
    grid = {}
    for late_a in range(0, 6):
        for late_b in range(0, 6):
            grid[late_a, late_b] = np.asarray(sref.cross_audit_slack(pa, la, pb, lb, 0.15, late_a, late_b, 0)[0])
    strictly = 0
    for (late_a, late_b), c in grid.items():
        for nxt in ((late_a + 1, late_b), (late_a, late_b + 1)):
            if nxt in grid:
                assert (grid[nxt] <= c).all(), (late_a, late_b, nxt)
                strictly += int((grid[nxt] < c).sum())
    assert strictly > 0, "the inputs were meant to have pairs for which the slack matters"


def test_slack_of_cap_or_more_is_the_minimum_over_every_pair_of_steps():
    cap = 13
    pa, la, pb, lb = _random_ragged(5, 4, 4, cap)
    full = sref.cross_audit_slack(pa, la, pb, lb, 0.15, cap, cap, 0)
    for late in ((cap + 1, cap), (10 ** 6, 10 ** 6), (cap - 1, cap - 1)):      # K - 1 already admits every pair
        got = sref.cross_audit_slack(pa, la, pb, lb, 0.15, late[0], late[1], 0)
        assert (_bits(got[0]) == _bits(full[0])).all() and got[1:] == full[1:]
    for i in range(4):
        for j in range(4):
            n, m = la[i], lb[j]
            if n == 0 or m == 0:
                assert full[0][i][j] == INF
                continue
            big_k = max(n, m)
            d2 = [[ref.squared_distance(pa[i][min(k, n - 1)], pb[j][min(l, m - 1)], 0) for l in range(big_k)] for k in range(big_k)]
            least = min(min(row) for row in d2)
            assert full[0][i][j] == math.sqrt(least) - 0.15
            k, l = full[1][i][j], full[2][i][j]
            assert d2[k][l] == least
            assert (k, l) == min((k, l) for k in range(big_k) for l in range(big_k) if d2[k][l] == least)


@pytest.mark.parametrize("late", [(0, 0), (3, 2), (1, 7), (40, 0)])
def test_transposition_of_the_clearances(late):
    """audit(A, B, late_a, late_b) and audit(B, A, late_b, late_a): the clearances are transposes bit for bit. The steps
    are where the minimum is unique -- which they are here for most pairs, and are not for the held ends."""
    pa, la, pb, lb = _random_ragged(6, 5, 4, 15)
    c, sa, sb = sref.cross_audit_slack(pa, la, pb, lb, 0.15, late[0], late[1], 0)
    ct, sat, sbt = sref.cross_audit_slack(pb, lb, pa, la, 0.15, late[1], late[0], 0)
    assert (_bits(c) == _bits(np.asarray(ct).T)).all()
    same = (np.asarray(sa) == np.asarray(sbt).T) & (np.asarray(sb) == np.asarray(sat).T)
    print("pairs whose steps transpose:", int(same.sum()), "of", same.size)
    assert same.sum() > same.size // 2


def test_steps_need_not_transpose_where_the_minimum_ties():
    """the least distance is reached at (0, 1) and at (1, 0): either scan reports the pair with ITS smaller first step"""
    a = [(0.0, 0.0, 0.0), (10.0, 0.0, 0.0)]
    b = [(10.0, 0.0, 0.0), (0.0, 0.0, 0.0)]
    assert sref.pair_clearance_slack(a, b, 0.0, 1, 1, 0) == (0.0, 0, 1)
    assert sref.pair_clearance_slack(b, a, 0.0, 1, 1, 0) == (0.0, 0, 1)       # i.e. A's step 1, B's step 0: not the transpose


def test_python_layer_has_the_calls(pmaf):
    names = {"pmaf_cross_audit_slack", "pmaf_cross_audit_tracks_slack", "pmaf_select_pair_slack"}
    assert names <= set(pmaf.planner.SYMBOLS)
    for m in ("cross_audit_slack", "cross_audit_tracks_slack", "select_pair_slack"):
        assert callable(getattr(pmaf.PmafPlanner, m))
    import inspect
    assert inspect.signature(pmaf.shard.DualArmCoupling.pair_tick).parameters["late"].default is None


def test_library_exports_the_calls(hip_lib):
    for name in ("pmaf_cross_audit_slack", "pmaf_cross_audit_tracks_slack", "pmaf_select_pair_slack"):
        assert getattr(hip_lib, name) is not None


def test_the_kernel_is_its_own_and_uses_no_scratch(pmaf):
    """k_cross_audit_slack in the build's resource record: no scratch, no spills, several waves per SIMD, and an LDS
    footprint that is the un-slacked kernel's (it does not depend on the slack)"""
    rec = os.path.join(os.path.dirname(pmaf.LIB_PATH), "resource_usage.txt")
    if not os.path.exists(rec):
        pytest.skip("no resource record next to the library (built by another recipe)")
    blocks = {b.split()[0]: b for b in open(rec).read().split("Function Name: ")[1:]}
    slack = [b for k, b in blocks.items() if "k_cross_audit_slack" in k]
    plain = [b for k, b in blocks.items() if re.search(r"\d+k_cross_auditE", k)]
    assert len(slack) == 1 and len(plain) == 1, sorted(blocks)

    def field(b, name):
        return int(re.search(re.escape(name) + r": (\d+)", b).group(1))
    print(slack[0])
    assert field(slack[0], "ScratchSize [bytes/lane]") == 0
    assert field(slack[0], "VGPRs Spill") == 0 and field(slack[0], "SGPRs Spill") == 0
    assert field(slack[0], "Occupancy [waves/SIMD]") >= 4
    assert field(slack[0], "LDS Size [bytes/block]") == field(plain[0], "LDS Size [bytes/block]")


CALLER = r'''
#include "bimanual_planning_ros/cf_manager.h"
using namespace ghostplanner::cfplanner;
CrossAudit (CfManager::*const kPlain)(const std::vector<std::vector<Vector3d>> &, double) = &CfManager::crossAudit;
CrossAudit (CfManager::*const kSlack)(const std::vector<std::vector<Vector3d>> &, double, int, int) = &CfManager::crossAudit;
double closest(CfManager &left, CfManager &right, int &agent, int &other, int &step, int &other_step) {
  const CrossAudit r = left.crossAudit(right.getPredictedPaths(), 0.15, 3, 2);
  double least = r.at(0, 0);
  agent = other = 0;
  for (int i = 0; i < r.n_agents; ++i)
    for (int j = 0; j < r.n_other; ++j)
      if (r.at(i, j) < least) { least = r.at(i, j); agent = i; other = j; }
  step = r.step_at(agent, other);
  other_step = r.other_step_at(agent, other);
  return least + r.other_step.at(0);
}
'''


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_overload_compiles(eigen):
    """CfManager::crossAudit with the two slacks through a compiler, next to the overload without (which must still
    resolve): plain build and the PMAF_USE_EIGEN branch, the way tests/test_cross_audit.py builds its unit"""
    chk = os.path.join(ROOT, "tests", "cpp", "eigen_api_check")
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")]
    if eigen:
        cmd += ["-DPMAF_USE_EIGEN", "-I" + chk, "-I" + os.path.join(chk, "eigen3")]
    r = subprocess.run(cmd + ["-x", "c++", "-"], input=CALLER.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
