"""The audits against the obstacle tracks (include/pmaf.h: pmaf_evaluate_paths_tracked, pmaf_select_clear_tracked)
without a device: tests/tracked_audit_reference.py is shown to be the untracked references on straight-line tracks, every
shape group the GPU suite runs (tests/test_tracked_audit_gpu.py) is shown to be sensitive to each rule of the contract,
and the new kernels' resource record is held to no scratch. The paths are the oracle's rollouts as
tests/test_field_track.py makes them."""
import os
import re

import numpy as np
import pytest

import field_track_reference as fref
import path_audit_reference as par
import select_clear_reference as sref
import tracked_audit_reference as ref
from test_field_track import _case_tracks, composed, untracked

INT32_MAX = 2 ** 31 - 1


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


def live_list(sc, paths, n_points):
    """the list of the tick after the reset: the field obstacles have moved on and drift, their radii are not the
    creation list's, and the trailing obstacle -- a small sphere at rest -- sits ON agent 1's path, half way"""
    live = np.array(sc["obstacles"], dtype=np.float64, copy=True)
    M = len(live) - 1
    live[:M, 0:3] += 0.01
    live[:M, 3:6] += 0.02 * np.cos(np.arange(M)[:, None] + np.arange(3)[None, :])
    live[:M, 6] *= 1.1
    k = int(n_points[1]) // 2
    live[M] = [paths[1][k][0], paths[1][k][1], paths[1][k][2], 0.0, 0.0, 0.0, 0.02]
    return live


def tables(run):
    """one population's rollout as the references' [P][N]... lists"""
    return [np.asarray(run["paths"]).tolist()], [np.asarray(run["n_points"]).tolist()], [np.asarray(run["costs"]).tolist()]


def both(paths, n, costs, live, tracks, first, sc, order, horizon, skip, mutant=None, margin=0.0):
    """(the tracked audit, the tracked selection) of one population"""
    a = ref.audit(paths, n, [live.tolist()], [tracks], [first], sc["dt"], sc["radius"], margin, order, mutant=mutant)
    s = ref.select_clear(paths, n, [live.tolist()], [tracks], [first], costs, sc["dt"], sc["radius"], margin, horizon, skip,
                         order, prev=[1], mutant=mutant)
    return a, s


@pytest.mark.parametrize("shape", list(fref.SHAPES))
def test_straight_line_tracks_give_the_untracked_references(oracle, scenes, shape):
    """tracks that are the list's iterated lines (cap + 5 points): path_audit_reference.audit and
    select_clear_reference.select_clear exactly; and the same with no tracks"""
    sc = fref.build_scene(scenes, shape)
    run = untracked(oracle, sc)
    paths, n, costs = tables(run)
    live = live_list(sc, paths[0], n[0])
    cap, order = sc["max_prediction_steps"], oracle.eval_order()
    lines = fref.straight_lines(live, sc["dt"], cap + 5).tolist()
    want_a = par.audit(paths, n, [live.tolist()], sc["dt"], sc["radius"], 0.02, order)
    for tracks in (lines, None, []):
        got_a = ref.audit(paths, n, [live.tolist()], [tracks], [0], sc["dt"], sc["radius"], 0.02, order)
        assert got_a == want_a
        for horizon in (1, 3, cap // 2, cap):
            for prev in (None, [2]):
                want_s = sref.select_clear(paths, n, [live.tolist()], costs, sc["dt"], sc["radius"], 0.02, horizon, order, prev)
                got_s = ref.select_clear(paths, n, [live.tolist()], [tracks], [0], costs, sc["dt"], sc["radius"], 0.02, horizon,
                                         False, order, prev)
                assert got_s == want_s
    # the trailing obstacle sits on agent 1's path: leaving it out is seen
    with_it = ref.window_audit(paths, n, [live.tolist()], [lines], [0], sc["dt"], sc["radius"], 0.02, cap, False, order)
    without = ref.window_audit(paths, n, [live.tolist()], [lines], [0], sc["dt"], sc["radius"], 0.02, cap, True, order)
    assert with_it[0][0][1] < 0.0 < without[0][0][1]


def test_an_offset_past_the_end_is_the_last_point():
    for L in (1, 2, 9):
        for k in (0, 1, 8, 69):
            assert ref.point_index(INT32_MAX, k, L) == L - 1
            assert ref.point_index(L + 3, k, L) == L - 1
            assert ref.point_index(L - 1, k, L) == L - 1
            assert ref.point_index(0, k, L) == min(k, L - 1)


CASES_FIRST = (("short", 0), ("short", "L-1"), ("Lcap", 1), ("L2", 1), ("Lcap+5", 0))
CASES_OTHER = (("short", 0), ("Lcap", 1))


@pytest.mark.parametrize("group", list(fref.SHAPE_GROUPS))
def test_cases_are_sensitive(oracle, scenes, group):
    """every mutant of the contract changes an output of the audit or of the selection in at least one case of every
    shape group, every case sees at least one of them, and every case differs from the untracked calls' result"""
    order = oracle.eval_order()
    hit = {m: 0 for m in ref.MUTANTS}
    for j, shape in enumerate(fref.SHAPE_GROUPS[group]):
        sc, un, tracks = _case_tracks(oracle, scenes, shape)
        cap = sc["max_prediction_steps"]
        for tname, first in (CASES_FIRST if j == 0 else CASES_OTHER):
            t = tracks[tname]
            f = fref.resolve_first(first, len(t))
            paths, n, costs = tables(composed(oracle, sc, t, f))
            live = live_list(sc, paths[0], n[0])
            tl = np.asarray(t).tolist()
            want = both(paths, n, costs, live, tl, f, sc, order, cap, False)
            plain = (par.audit(paths, n, [live.tolist()], sc["dt"], sc["radius"], 0.0, order),
                     sref.select_clear(paths, n, [live.tolist()], costs, sc["dt"], sc["radius"], 0.0, cap, order, [1]))
            assert want[0] != plain[0], (shape, tname, first)
            seen = 0
            for m in ref.MUTANTS:
                got = both(paths, n, costs, live, tl, f, sc, order, cap, False, mutant=m)
                if got != want:
                    hit[m] += 1
                    seen += 1
            assert seen >= 1, (shape, tname, first)
    assert all(v >= 1 for v in hit.values()), hit


def test_auditft_kernels_use_no_scratch(pmaf, hip_lib):
    path = os.path.join(os.path.dirname(os.path.abspath(pmaf.LIB_PATH)), "resource_usage.txt")
    text = open(path).read()
    blocks = re.split(r"(?=Function Name: )", text)
    mine = [b for b in blocks if re.match(r"Function Name: _Z\d+k_(ft_select_audit|audit_track_ft)", b)]
    assert len(mine) == 2, [b.splitlines()[0] for b in mine]
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b
        assert re.search(r"VGPRs Spill: 0\b", b), b
        assert re.search(r"SGPRs Spill: 0\b", b), b
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        assert occ >= 4, b   # no chain to hide: the audit relies on occupancy, as k_path_audit does
