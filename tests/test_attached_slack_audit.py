"""The reference of the joint selection on coupled handles with timing slack (tests/attached_slack_reference.py) on the
CPU: at (0, 0) it is attached_audit_reference exactly, without attachments slack_audit_reference exactly; the clearance
never grows with a slack; a call and its transposed call have the same clearance bits; every mutant of the contract
changes an output in every shape group the GPU suite runs; in every group a sphere term wins a pair at two different
steps; and the pre-conditions of the GPU suite's behavioural case hold on the same scenes, so that it cannot pass
vacuously. The paths are the oracle's rollouts of tests/attached_slack_cases.py's scenes. Also the binding table, the
header and the new kernel's resource record."""
import os
import re

import numpy as np
import pytest

import attached_audit_reference as aar
import attached_slack_cases as cases
import attached_slack_reference as ref
import conftest
import pair_clear_reference as pcr
import slack_audit_reference as sar
from test_attached_audit import oracle_tables, stale_tracks, tie_separation

ROOT = conftest.ROOT
INF = float("inf")
N5 = [s for s in cases.SHAPES if cases.SHAPES[s]["N"] == 5]


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


_LATE = {}


def tables_of(oracle, scenes, shape):
    """test_attached_audit.oracle_tables, and the same of the behavioural shape: (scenes, paths, n, costs, live), computed
    once per session and never modified"""
    if shape != cases.LATE_SHAPE:
        return oracle_tables(oracle, scenes, shape)
    key = oracle.eval_order()
    if key not in _LATE:
        scs = cases.build_scenes(scenes, shape)
        paths, n, costs = [], [], []
        for sc in scs:
            o = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
            try:
                o.set_initial_position(sc["start"])
                o.rollout()
                o.evaluate(sc["cost_gains"], sc["ws_limits"])
                pp, nn = o.paths()
                paths.append(np.asarray(pp).reshape(5, -1, 3).tolist())
                n.append(np.asarray(nn).reshape(5).tolist())
                costs.append(np.asarray(o.costs()).reshape(5).tolist())
            finally:
                o.close()
        _LATE[key] = (scs, paths, n, costs, cases.live_list(scenes, scs).tolist())
    return _LATE[key]


def whole(tables, cpl, late, order, mutant=None, sep=cases.SEP, a=0, b=1):
    scs, paths, n, costs, live = tables
    return ref.cross_audit_attached_slack(paths[a], n[a], paths[b], n[b], cpl, a, b, live, scs[0]["radius"], sep, late[0],
                                          late[1], order, mutant)


@pytest.mark.parametrize("shape", N5)
def test_at_0_0_the_reference_is_the_attached_reference(oracle, scenes, shape):
    tables = tables_of(oracle, scenes, shape)
    scs, paths, n, costs, live = tables
    order = oracle.eval_order()
    for kind in cases.kinds(shape):
        cpl = cases.coupling(shape, kind, scs)
        seps = (cases.SEP, tie_separation(scs, live)) if kind == "tie" else (cases.SEP,)
        for sep in seps:
            clr, sa, sb, sp = whole(tables, cpl, (0, 0), order, sep=sep)
            want = aar.cross_audit_attached(paths[0], n[0], paths[1], n[1], cpl, 0, 1, live, scs[0]["radius"], sep, order)
            assert (clr, sa, sp) == want and sb == sa, (shape, kind)


@pytest.mark.parametrize("shape", N5)
def test_without_attachments_the_reference_is_the_slacked_reference(oracle, scenes, shape):
    tables = tables_of(oracle, scenes, shape)
    scs, paths, n, costs, live = tables
    order = oracle.eval_order()
    s = cases.SHAPES[shape]
    idle = dict(src=np.full((s["P"], s["M"]), -1), scale=np.ones((s["P"], s["M"])), anchor=np.zeros((s["P"], s["M"], 3)), shift=0)
    for late in cases.slacks(s["cap"])[:-1]:
        want = sar.cross_audit_slack(paths[0], n[0], paths[1], n[1], cases.SEP, late[0], late[1], order)
        for cpl in (None, idle):
            clr, sa, sb, sp = whole(tables, cpl, late, order)
            assert (clr, sa, sb) == want, (shape, late)
            assert sp == [[0 if k >= 0 else -1 for k in row] for row in sa]


@pytest.mark.parametrize("shape", ["P2-N5-M3-cap9", "P2-N5-M3-cap70-ragged", cases.LATE_SHAPE])
def test_the_clearance_never_grows_with_a_slack(oracle, scenes, shape):
    tables = tables_of(oracle, scenes, shape)
    order = oracle.eval_order()
    cap = cases.shape_of(shape)["cap"]
    base = "P2-N5-M3-cap9" if shape == cases.LATE_SHAPE else shape
    for kind in ("one", "three"):
        cpl = cases.coupling(base, kind, tables[0])
        prev, fell = None, 0
        for late in cases.chain(cap):
            clr = whole(tables, cpl, late, order)[0]
            if prev is not None:
                for row, prow in zip(clr, prev):
                    for v, pv in zip(row, prow):
                        assert v <= pv, (shape, kind, late)
                        fell += v < pv
            prev = clr
        print(shape, kind, "clearances that fell along the chain:", fell)


@pytest.mark.parametrize("shape", ["P2-N5-M3-cap9", "P2-N5-M3-cap70-ragged", "P3-N5-M3-cap70-ragged"])
def test_the_transposed_call_has_the_transposed_clearance(oracle, scenes, shape):
    """audit(A, B, late_a, late_b) against audit(B, A, late_b, late_a): each sphere's u - z is the same vector in both
    calls, so every d2, every gap and the minimum have the same bits; the codes swap 1 + s <-> 1 + M + s (where no two
    terms tie in the gap: not in kind `tie`). The steps transpose only where the minimum is unique: not compared."""
    tables = tables_of(oracle, scenes, shape)
    scs = tables[0]
    order = oracle.eval_order()
    M = cases.SHAPES[shape]["M"]
    for kind in ("one", "tie", "three"):
        cpl = cases.coupling(shape, kind, scs)
        for late in ((0, 0), (3, 2), (0, 2 * cases.C + 3)):
            clr, sa, sb, sp = whole(tables, cpl, late, order, a=0, b=1)
            tlr, ta, tb, tp = whole(tables, cpl, (late[1], late[0]), order, a=1, b=0)
            for i in range(5):
                for j in range(5):
                    assert clr[i][j] == tlr[j][i], (shape, kind, late, i, j)
                    if kind != "tie":
                        c = sp[i][j]
                        swapped = c if c <= 0 else (c + M if c <= M else c - M)
                        assert tp[j][i] == swapped, (shape, kind, late, i, j)


def answers(tables, cpl, tracks, order, mutant, sep, cache):
    """what the GPU suite compares, for one coupling: the matrices on the whole paths at three slacks and the joint
    selection at (3, 2) on a window inside the paths, both skip settings, two pairs of margins"""
    scs, paths, n, costs, live = tables
    dt, rad, cap = scs[0]["dt"], scs[0]["radius"], scs[0]["max_prediction_steps"]
    out = [whole(tables, cpl, late, order, mutant, sep) for late in ((1, 0), (3, 2), (0, 5))]
    horizon, late = max(4, cap // 3), (3, 2)
    mat = ref.pair_side(paths[0], n[0], paths[1], n[1], cpl, 0, 1, live, rad, horizon, sep, late, order, mutant)
    for skip in (0, 1):
        for om, pm in ((-0.5, -0.5), (0.02, 0.0)):
            ka = (om, horizon, skip)
            if ka not in cache:
                cache[ka] = aar.obstacle_side(paths, n, live, tracks, None, cpl, 0, 1, dt, rad, om, horizon, skip, order)
            out.append(ref.select_pair_clear_tracked_slack(paths, n, live, tracks, None, cpl, costs, dt, rad, 0, 1, om, horizon,
                                                           skip, sep, pm, late, (1, 2), order, cache[ka], mat))
    return out


GROUP_SHAPES = {g: tuple(v) for g, v in cases.SHAPE_GROUPS.items()}


@pytest.mark.parametrize("group", list(GROUP_SHAPES))
def test_every_mutant_changes_an_output_in_every_shape_group(oracle, scenes, group):
    order = oracle.eval_order()
    hit = {m: 0 for m in ref.MUTANTS}
    for shape in GROUP_SHAPES[group]:
        tables = tables_of(oracle, scenes, shape)
        scs, paths, n, costs, live = tables
        for kind in ("one", "tie", "three"):      # (`all`, 61 terms in plain Python, is the GPU suite's own)
            cpl = cases.coupling(shape, kind, scs)
            tracks = stale_tracks(scs, paths, n, costs, cpl)
            sep = tie_separation(scs, live) if kind == "tie" else cases.SEP
            cache = {}
            want = answers(tables, cpl, tracks, order, None, sep, cache)
            seen = []
            for m in ref.MUTANTS:
                if answers(tables, cpl, tracks, order, m, sep, cache) != want:
                    hit[m] += 1
                    seen.append(m)
            print(shape, kind, "mutants seen:", seen)
    # a tie inside a term: the group's first shape with population 0's paths on both sides (cases.twin_coupling)
    shape = GROUP_SHAPES[group][0]
    scs, paths, n, costs, live = tables_of(oracle, scenes, shape)
    twin = (scs, [paths[0]] * len(paths), [n[0]] * len(n), [costs[0]] * len(costs), live)
    cpl, ka, kb = cases.twin_coupling(cases.SHAPES[shape]["P"], cases.SHAPES[shape]["M"], twin[1], twin[2], 0)
    want = whole(twin, cpl, (3, 2), order, sep=cases.TWIN_SEP)
    print("twin steps", ka, kb, "pair (0, 0):", [m[0][0] for m in want])
    assert (want[1][0][0], want[2][0][0], want[3][0][0]) == (ka, kb, 1) and want[0][0][0] < -cases.TWIN_SEP
    seen = [m for m in ref.MUTANTS if whole(twin, cpl, (3, 2), order, m, sep=cases.TWIN_SEP) != want]
    assert "tie_lk" in seen
    print(shape, "twin", "mutants seen:", seen)
    for m in seen:
        hit[m] += 1
    assert all(v >= 1 for v in hit.values()), hit


@pytest.mark.parametrize("group", list(GROUP_SHAPES))
def test_a_sphere_term_wins_at_two_different_steps_in_every_group(oracle, scenes, group):
    """at (3, 2): at least one pair is won by a sphere term with step_a != step_b -- the suite cannot pass on inputs on
    which the slack never matters to a sphere"""
    order = oracle.eval_order()
    count = 0
    for shape in GROUP_SHAPES[group]:
        tables = tables_of(oracle, scenes, shape)
        for kind in ("one", "three"):
            cpl = cases.coupling(shape, kind, tables[0])
            clr, sa, sb, sp = whole(tables, cpl, (3, 2), order)
            here = sum(1 for i in range(5) for j in range(5) if sp[i][j] > 0 and sa[i][j] != sb[i][j])
            print(shape, kind, "pairs won by a sphere term at two different steps:", here)
            count += here
    print(group, "total:", count)
    assert count >= 1


# ---- the pre-conditions of the GPU suite's behavioural case ----
BEHAVIOUR = dict(obstacle_margin=-0.5, pair_margin=0.0, skip_trailing=1)


@pytest.mark.parametrize("side", [0, 1])
def test_preconditions_of_the_behavioural_gpu_case(oracle, scenes, side):
    """on the dt = 0.1 shape the un-slacked tracked reference returns (i*, j*) although a sphere riding on one member sits,
    d steps later, on the other member's point; the slacked reference at the revealing slack returns another pair or
    rule 2; the same lag the wrong way round keeps (i*, j*)"""
    scs, paths, n, costs, live = tables_of(oracle, scenes, cases.LATE_SHAPE)
    order = oracle.eval_order()
    dt, rad, cap = scs[0]["dt"], scs[0]["radius"], scs[0]["max_prediction_steps"]
    assert dt == 0.1 and cap == cases.LATE_CAP
    b, d = BEHAVIOUR, cases.LATE_D
    plain = pcr.select_pair_clear(paths, n, live, costs, dt, rad, 0, 1, b["obstacle_margin"], cap, b["skip_trailing"], cases.SEP,
                                  b["pair_margin"], None, None, order)
    assert plain["rule"] in (0, 1) and plain["pair"][0] >= 0, plain
    star = plain["pair"]
    k = cases.late_step(n)
    assert k >= 1
    cpl = cases.sphere_on_the_late_pair(2, 3, paths, n, star, k, d, side)
    far = cases.late_rows(np.asarray(live), cpl).tolist()
    args = (paths, n, far, None, None, cpl, costs, dt, rad, 0, 1, b["obstacle_margin"], cap, b["skip_trailing"], cases.SEP,
            b["pair_margin"])
    tracked = aar.select_pair_clear_tracked(*args, None, order)
    i, j = star
    gaps = {late: ref.attached_slack_pair(paths[0][i][:n[0][i]], paths[1][j][:n[1][j]],
                                          aar.terms_of(cpl, 0, 1, far, rad, cases.SEP), late[0], late[1], order)
            for late in ((0, 0), cases.late_slack(side), cases.late_slack(side, wrong=True))}
    hit = ref.select_pair_clear_tracked_slack(*args, cases.late_slack(side), None, order)
    wrong = ref.select_pair_clear_tracked_slack(*args, cases.late_slack(side, wrong=True), None, order)
    print("side", side, "k", k, "untracked", plain["pair"], plain["rule"], plain["n_feasible"], "tracked", tracked["pair"],
          tracked["rule"], tracked["n_feasible"], "slacked", hit["pair"], hit["rule"], hit["n_feasible"], "wrong way",
          wrong["pair"], wrong["rule"], wrong["n_feasible"])
    print("gaps of the pair:", gaps)
    assert tracked["pair"] == star and tracked["rule"] in (0, 1)
    assert hit["pair"] != star or hit["rule"] == 2
    assert hit["pair"] != star, "the pair whose late arm runs into the sphere must not be returned"
    assert wrong["pair"] == star
    g = gaps[cases.late_slack(side)]
    assert g[0] < 0.0 and g[3] == (1 if side == 0 else 1 + 3)
    assert (g[1], g[2]) == ((k, k + d) if side == 0 else (k + d, k))
    assert gaps[(0, 0)][0] > 0.0


# ---- the binding table, the header, the resource record ----
def test_binding_table_lists_the_exports(pmaf):
    assert {"pmaf_cross_audit_attached_slack", "pmaf_select_pair_clear_tracked_slack"} <= set(pmaf.planner.SYMBOLS)
    assert callable(getattr(pmaf.PmafPlanner, "cross_audit_attached_slack"))
    import inspect
    assert "late" in inspect.signature(pmaf.PmafPlanner.select_pair_clear_tracked).parameters


def test_header_keeps_abi_7_and_declares_the_exports():
    hdr = open(os.path.join(ROOT, "include", "pmaf.h")).read()
    assert "#define PMAF_ABI_VERSION 7" in hdr
    for name in ("pmaf_cross_audit_attached_slack", "pmaf_select_pair_clear_tracked_slack"):
        assert "int %s(pmaf_planner *h" % name in hdr
    assert "no `late`" not in hdr


def test_resource_record_of_the_new_kernel(pmaf, hip_lib):
    """k_xaudit_attached_slack: no scratch, no spills, the tile's LDS whatever the slack and the number of terms"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(pmaf.LIB_PATH)), "resource_usage.txt")).read()
    blocks = {b.splitlines()[0]: b for b in re.split(r"(?=Function Name: )", text) if b.startswith("Function Name:")}
    mine = [b for k, b in blocks.items() if re.search(r"\d+k_xaudit_attached_slack", k)]
    assert len(mine) == 1, sorted(blocks)
    print(mine[0])
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", mine[0]), mine[0]
    assert re.search(r"VGPRs Spill: 0\b", mine[0]) and re.search(r"SGPRs Spill: 0\b", mine[0]), mine[0]
    lds = lambda b: int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
    plain = [b for k, b in blocks.items() if re.search(r"\d+k_cross_auditE", k)]
    assert len(plain) == 1 and lds(mine[0]) == lds(plain[0]) == 25608
