"""The audits against the live list with timing slack (include/pmaf.h: pmaf_evaluate_paths_slack,
pmaf_select_clear_slack) without a device: tests/obstacle_slack_reference.py is shown to be the tracked and the untracked
references at (late, early) = (0, 0), the contract's monotonicity consequences are shown to hold, every shape group the
GPU suite runs (tests/test_obstacle_slack_audit_gpu.py) is shown to be sensitive to each rule of the contract, the header
and the binding table are held to the two exports, and the new kernels' resource record to no scratch. The paths are the
oracle's rollouts as tests/test_field_track.py makes them."""
import os
import re

import numpy as np
import pytest

import field_track_reference as fref
import obstacle_slack_reference as ref
import path_audit_reference as par
import select_clear_reference as sref
import tracked_audit_reference as tref
from test_field_track import _case_tracks, composed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIT_KEYS = ("clearance", "step", "obstacle", "first_violation")


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


def tables(run):
    """one population's rollout as the references' [P][N]... lists"""
    return [np.asarray(run["paths"]).tolist()], [np.asarray(run["n_points"]).tolist()], [np.asarray(run["costs"]).tolist()]


def live_list(sc, paths, n_points, late=2):
    """the list of the tick after the reset: the field obstacles have moved on and drift, their radii are not the
    creation list's, and the trailing obstacle -- a small MOVING sphere -- reaches agent 1's path point k*, half way, at
    the obstacles' index k* + late: step against step it passes behind the arm, an arm `late` steps late is hit"""
    live = np.array(sc["obstacles"], dtype=np.float64, copy=True)
    M = len(live) - 1
    live[:M, 0:3] += 0.01
    live[:M, 3:6] += 0.02 * np.cos(np.arange(M)[:, None] + np.arange(3)[None, :])
    live[:M, 6] *= 1.1
    k = int(n_points[1]) // 2
    v = np.array([0.9, -1.3, 0.7])
    at = np.asarray(paths[1][k], dtype=np.float64)
    for _ in range(k + late):
        at = at - v * sc["dt"]
    live[M] = [at[0], at[1], at[2], v[0], v[1], v[2], 0.02]
    return live


def constructed(tracks, paths, n_points, first):
    """the case's tracks with three exact hits of obstacle 0 (c = -(radius + r), the least a pair can give) where the
    window allows them, all read from the offset `first`:
      a tie between two (k, l) pairs of agent 0: index 3 = its point 2, index 2 = its point 3 (needs late, early >= 1);
      index 0 = agent 2's point 1: the winner (1, 0) lies on the l >= 0 edge of the band (needs early >= 1);
      the point before the last = agent 3's point k = L - f + 2, which reads the held end at every index of a band of
      early <= 3: no admitted pair meets it, and a hold applied before the slack does (needs a track that ends mid-path)"""
    t = np.array(tracks, dtype=np.float64, copy=True)
    L = len(t)
    f = min(first, L - 1)
    if L - f >= 4 and n_points[0] >= 4:
        t[f + 3, 0, 0:3] = paths[0][2]
        t[f + 2, 0, 0:3] = paths[0][3]
    if n_points[2] >= 2:
        t[f, 0, 0:3] = paths[2][1]
    if L - f >= 6 and n_points[3] > L - f + 2:
        t[L - 2, 0, 0:3] = paths[3][L - f + 2]
    return t.tolist()


def both(paths, n, costs, live, tracks, first, sc, order, horizon, skip, late, early, mutant=None, margin=0.0):
    """(the slacked audit, the slacked selection) of one population"""
    a = ref.audit(paths, n, [live.tolist()], [tracks], [first], sc["dt"], sc["radius"], margin, late, early, order, mutant=mutant)
    s = ref.select_clear(paths, n, [live.tolist()], [tracks], [first], costs, sc["dt"], sc["radius"], margin, horizon, skip,
                         late, early, order, prev=[1], mutant=mutant)
    return a, s


def _cases(oracle, scenes, shape, names):
    """(sc, paths, n, costs, live, tracks or None, first) per named track of a shape; None: the untracked rollout"""
    sc, un, tracks = _case_tracks(oracle, scenes, shape)
    out = []
    for name, first in names:
        if name is None:
            paths, n, costs = tables(un)
            out.append((sc, paths, n, costs, live_list(sc, paths[0], n[0]), None, 0))
            continue
        t = tracks[name]
        f = fref.resolve_first(first, len(t))
        paths, n, costs = tables(composed(oracle, sc, t, f))
        out.append((sc, paths, n, costs, live_list(sc, paths[0], n[0]), constructed(t, paths[0], n[0], f), f))
    return out


@pytest.mark.parametrize("group", list(fref.SHAPE_GROUPS))
def test_zero_slack_is_the_unslacked_references(oracle, scenes, group):
    """(late, early) = (0, 0): tracked_audit_reference's audit and selection bit for bit with obstacle_step == step; and
    without tracks path_audit_reference's and select_clear_reference's"""
    order = oracle.eval_order()
    for j, shape in enumerate(fref.SHAPE_GROUPS[group]):
        names = ((None, 0), ("short", 1), ("Lcap", "L-1"), ("L2", 0)) if j == 0 else ((None, 0), ("short", 0))
        for sc, paths, n, costs, live, tracks, f in _cases(oracle, scenes, shape, names):
            cap, ll = sc["max_prediction_steps"], [live.tolist()]
            got = ref.audit(paths, n, ll, [tracks], [f], sc["dt"], sc["radius"], 0.02, 0, 0, order)
            want = tref.audit(paths, n, ll, [tracks], [f], sc["dt"], sc["radius"], 0.02, order)
            for k in AUDIT_KEYS:
                assert got[k] == want[k], (shape, k)
            assert got["obstacle_step"] == got["step"]
            if tracks is None:
                plain = par.audit(paths, n, ll, sc["dt"], sc["radius"], 0.02, order)
                for k in AUDIT_KEYS:
                    assert got[k] == plain[k], (shape, k)
            for horizon in (1, 3, cap):
                for skip in (False, True):
                    s = ref.select_clear(paths, n, ll, [tracks], [f], costs, sc["dt"], sc["radius"], 0.02, horizon, skip, 0, 0,
                                         order, prev=[2])
                    t = tref.select_clear(paths, n, ll, [tracks], [f], costs, sc["dt"], sc["radius"], 0.02, horizon, skip, order,
                                          prev=[2])
                    assert s == t, (shape, horizon, skip)
                    if tracks is None and not skip:
                        assert s == sref.select_clear(paths, n, ll, costs, sc["dt"], sc["radius"], 0.02, horizon, order, [2])


BANDS = ((0, 0), (1, 0), (0, 1), (2, 3), (75, 75))


@pytest.mark.parametrize("shape", ["M3-cap70", "M59-cap9-general-moving"])
def test_nothing_grows_with_either_slack(oracle, scenes, shape):
    """clearance, first_violation and n_clear never grow when either slack grows; a slack above max_prediction_steps is
    max_prediction_steps"""
    order = oracle.eval_order()
    for sc, paths, n, costs, live, tracks, f in _cases(oracle, scenes, shape, ((None, 0), ("short", 1))):
        cap = sc["max_prediction_steps"]
        res = {}
        for late, early in BANDS + ((cap, cap),):
            res[(late, early)] = both(paths, n, costs, live, tracks, f, sc, order, cap, False, late, early, margin=0.05)
        assert res[(75, 75)] == res[(cap, cap)]
        for small in res:
            for big in res:
                if big[0] >= small[0] and big[1] >= small[1]:
                    (a0, s0), (a1, s1) = res[small], res[big]
                    for c0, c1 in zip(a0["clearance"][0], a1["clearance"][0]):
                        assert c1 <= c0, (small, big)
                    for v0, v1 in zip(a0["first_violation"][0], a1["first_violation"][0]):
                        assert v1 <= v0, (small, big)
                    assert s1["n_clear"][0] <= s0["n_clear"][0], (small, big)


def test_a_list_at_rest_without_tracks_gives_the_unslacked_bits(oracle, scenes):
    """every index of an obstacle at rest is one place: clearance, step, obstacle, first_violation and the selection are
    those of (0, 0) for every slack; obstacle_step is the band's first index max(step - early, 0)"""
    order = oracle.eval_order()
    sc, paths, n, costs, live, _, _ = _cases(oracle, scenes, "M3-cap70", ((None, 0),))[0]
    live = live.copy()
    live[:, 3:6] = 0.0
    want = both(paths, n, costs, live, None, 0, sc, order, 50, False, 0, 0, margin=0.05)
    for late, early in BANDS[1:]:
        got = both(paths, n, costs, live, None, 0, sc, order, 50, False, late, early, margin=0.05)
        for k in AUDIT_KEYS:
            assert got[0][k] == want[0][k], (late, early, k)
        assert got[1] == want[1]
        ea = min(early, sc["max_prediction_steps"])
        assert got[0]["obstacle_step"][0] == [max(k - ea, 0) if k >= 0 else -1 for k in got[0]["step"][0]]


@pytest.mark.parametrize("group", list(fref.SHAPE_GROUPS))
def test_every_mutant_changes_an_output_in_every_shape_group(oracle, scenes, group):
    """every mutant of the contract changes an output of the audit or of the selection in at least one case of every
    shape group, and every case differs from the unslacked calls' result"""
    order = oracle.eval_order()
    hit = {m: 0 for m in ref.MUTANTS}
    for j, shape in enumerate(fref.SHAPE_GROUPS[group]):
        names = ((None, 0), ("short", 1), ("Lcap", 0)) if j == 0 else (("short", 0),)
        for sc, paths, n, costs, live, tracks, f in _cases(oracle, scenes, shape, names):
            cap = sc["max_prediction_steps"]
            for late, early in ((2, 3), (1, 1)) if j == 0 else ((2, 3),):
                want = both(paths, n, costs, live, tracks, f, sc, order, cap, False, late, early)
                plain = both(paths, n, costs, live, tracks, f, sc, order, cap, False, 0, 0)
                assert want != plain, (shape, late, early)
                for m in ref.MUTANTS:
                    if both(paths, n, costs, live, tracks, f, sc, order, cap, False, late, early, mutant=m) != want:
                        hit[m] += 1
    assert all(v >= 1 for v in hit.values()), hit


def test_the_moving_trailing_obstacle_hits_only_the_late_arm(oracle, scenes):
    """the live list's trailing sphere reaches agent 1's point k* at index k* + 2: clear of it step against step, hit with
    late = 2 at the ARM'S step k*, and not with early alone"""
    order = oracle.eval_order()
    sc, paths, n, costs, live, _, _ = _cases(oracle, scenes, "M3-cap70", ((None, 0),))[0]
    M, k = len(live) - 1, n[0][1] // 2
    r = {b: ref.audit(paths, n, [live.tolist()], None, None, sc["dt"], sc["radius"], 0.0, b[0], b[1], order) for b in
         ((0, 0), (2, 0), (0, 3), (1, 0))}
    hit = r[(2, 0)]
    assert (hit["step"][0][1], hit["obstacle_step"][0][1], hit["obstacle"][0][1]) == (k, k + 2, M)
    assert hit["clearance"][0][1] < -0.9 * (sc["radius"] + 0.02) and hit["first_violation"][0][1] <= k
    for b in ((0, 0), (0, 3), (1, 0)):
        assert r[b]["clearance"][0][1] > hit["clearance"][0][1]


def test_header_declares_both_exports_under_abi_7(pmaf):
    text = open(os.path.join(ROOT, "include", "pmaf.h")).read()
    assert re.search(r"^#define PMAF_ABI_VERSION 7\b", text, re.M)
    for name, n_args in (("pmaf_evaluate_paths_slack", 11), ("pmaf_select_clear_slack", 16)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        assert len(pmaf.planner.SYMBOLS[name][1]) == n_args, name   # the binding table
    block = text[text.index("clear selection with timing slack"):]
    block = block[:block.index("int pmaf_evaluate_paths_slack(")]
    m = re.search(r"Out of scope[^/]*?\*/|Out of scope.*?(?=\n \* Intended)", block, re.S)   # the out-of-scope paragraph
    assert m, "the header says what is out of scope"
    for word in ("per_obstacle", "pmaf_select_pair_clear", "pmaf_select_clear_tracks"):
        assert word in m.group(0), word


def test_obslack_kernels_use_no_scratch(pmaf, hip_lib):
    path = os.path.join(os.path.dirname(os.path.abspath(pmaf.LIB_PATH)), "resource_usage.txt")
    if not os.path.exists(path):
        pytest.skip("no resource record beside the library")
    blocks = re.split(r"(?=Function Name: )", open(path).read())
    mine = [b for b in blocks if re.match(r"Function Name: _Z\d+k_obs_slack_auditILb[01]E", b)]
    assert len(mine) == 2, [b.splitlines()[0] for b in mine]
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b
        assert re.search(r"VGPRs Spill: 0\b", b), b
        assert re.search(r"SGPRs Spill: 0\b", b), b
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        assert occ >= 4, b   # no chain to hide: the audit relies on occupancy, as k_select_audit does
