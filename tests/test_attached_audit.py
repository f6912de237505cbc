"""The reference of the joint selection on coupled handles (tests/attached_audit_reference.py) on the CPU: without
attachments it is the existing references exactly; a scale = 0 term is the path audit of a sphere at rest; every mutant
of the contract changes an output in every shape group the GPU suite runs; and the pre-conditions of the GPU suite's
behavioural cases hold on the same scenes, so that those cases cannot pass vacuously. The paths are the oracle's rollouts
of tests/attached_audit_cases.py's scenes. Also the binding table, the header and the new kernels' resource record."""
import os
import re

import numpy as np
import pytest

import attached_audit_cases as cases
import attached_audit_reference as ref
import conftest
import cross_audit_reference as car
import field_couple_reference as cref
import field_track_reference as fref
import pair_clear_reference as pcr
import path_audit_reference as par
import tracked_audit_reference as tar

ROOT = conftest.ROOT
INF = float("inf")


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


_TABLES = {}


def oracle_tables(oracle, scenes, shape):
    """(scenes, paths [P][N][cap][3], n [P][N], costs [P][N], live [P][n_obs][7]) of one shape: the oracle's rollouts,
    computed once per session and never modified"""
    key = (shape, oracle.eval_order())
    if key not in _TABLES:
        scs = cases.build_scenes(scenes, shape)
        N = cases.SHAPES[shape]["N"]
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
        _TABLES[key] = (scs, paths, n, costs, cases.live_list(scenes, scs).tolist())
    return _TABLES[key]


def stale_tracks(scs, paths, n, costs, cpl):
    """the tracks a launch in front of these rollouts would have composed from each arm's cheapest agent: what the
    obstacle side of a coupled population reads (stale for every other pair)"""
    if cpl is None:
        return None
    best = [int(np.argmin(c)) for c in costs]
    sel_p = [np.asarray(paths[q][best[q]]) for q in range(len(scs))]
    sel_n = [int(n[q][best[q]]) for q in range(len(scs))]
    out = []
    for p, sc in enumerate(scs):
        t = cref.compose_tracks(sel_p, sel_n, [True] * len(scs), cpl["src"][p], cpl["scale"][p], cpl["anchor"][p],
                                cpl["shift"], sc["obstacles"], sc["dt"], sc["max_prediction_steps"])
        out.append(t.tolist())
    return out


def tie_separation(scs, live):
    """the separation at which the first term of `tie` (arm 0's column 0: scale 1, anchor 0) ties with term 0 in the GAP
    as well. (Arm 1's column 0 has a smaller radius in these scenes, asserted where it matters: its gap is greater.)"""
    return float(scs[0]["radius"]) + float(live[0][0][6])


def answers(tables, cpl, tracks, order, mutant=None, sep=cases.SEP, cache=None):
    """what the GPU suite compares, for one coupling: the attached matrices on the whole paths and the joint selection
    over a few calls (horizons below and above the paths, both skip settings, two pairs of margins). cache: a dict shared
    by the calls of one coupling -- the obstacle side depends on two of the mutants only, the pair side not on the
    margins: each is computed once and never modified"""
    scs, paths, n, costs, live = tables
    dt, rad, cap = scs[0]["dt"], scs[0]["radius"], scs[0]["max_prediction_steps"]
    cache = {} if cache is None else cache
    out = [ref.cross_audit_attached(paths[0], n[0], paths[1], n[1], cpl, 0, 1, live, rad, sep, order, mutant)]
    for horizon in (max(2, cap // 3), cap + 3):
        km = ("pair", horizon, sep, mutant)
        if km not in cache:
            cache[km] = ref.pair_side(paths[0], n[0], paths[1], n[1], cpl, 0, 1, live, rad, horizon, sep, order, mutant)
        for skip in (0, 1):
            for om, pm in ((-0.5, -0.5), (0.02, 0.0)):
                ka = ("obstacle", om, horizon, skip, mutant if mutant in ("columns_kept", "ignored") else None)
                if ka not in cache:
                    cache[ka] = ref.obstacle_side(paths, n, live, tracks, None, cpl, 0, 1, dt, rad, om, horizon, skip, order, mutant)
                out.append(ref.select_pair_clear_tracked(paths, n, live, tracks, None, cpl, costs, dt, rad, 0, 1, om, horizon,
                                                         skip, sep, pm, (1, 2), order, cache[ka], cache[km]))
    return out


# (every shape but N = 33, whose 1 089 pairs are the GPU suite's own)
@pytest.mark.parametrize("shape", [s for s in cases.SHAPES if cases.SHAPES[s]["N"] == 5])
def test_without_attachments_the_reference_is_the_existing_references(oracle, scenes, shape):
    tables = oracle_tables(oracle, scenes, shape)
    scs, paths, n, costs, live = tables
    order = oracle.eval_order()
    dt, rad, cap = scs[0]["dt"], scs[0]["radius"], scs[0]["max_prediction_steps"]
    clr, step, sphere = ref.cross_audit_attached(paths[0], n[0], paths[1], n[1], None, 0, 1, live, rad, cases.SEP, order)
    assert (clr, step) == car.cross_audit(paths[0], n[0], paths[1], n[1], cases.SEP, order)
    assert sphere == [[0 if s >= 0 else -1 for s in row] for row in step]
    # a coupling in which nothing rides on the pair's populations is no attachment either
    P, M = cases.SHAPES[shape]["P"], cases.SHAPES[shape]["M"]
    idle = dict(src=np.full((P, M), -1), scale=np.ones((P, M)), anchor=np.zeros((P, M, 3)), shift=0)
    assert ref.cross_audit_attached(paths[0], n[0], paths[1], n[1], idle, 0, 1, live, rad, cases.SEP, order) == (clr, step, sphere)
    lines = [np.asarray(fref.straight_lines(np.asarray(live[p]), dt, cap + 2)).tolist() for p in range(P)]
    for horizon in (1, cap // 2, cap + 4):
        for skip in (0, 1):
            want_side = pcr.obstacle_side(paths, n, live, dt, rad, 0.02, horizon, skip, order)
            assert ref.obstacle_side(paths, n, live, None, None, None, 0, 1, dt, rad, 0.02, horizon, skip, order) == want_side
            # ... and on tracks, the tracked audit's
            assert ref.obstacle_side(paths, n, live, lines, None, None, 0, 1, dt, rad, 0.02, horizon, skip, order) == \
                tar.window_audit(paths, n, live, lines, None, dt, rad, 0.02, horizon, skip, order)
            for prev in (None, (1, 2)):
                want = pcr.select_pair_clear(paths, n, live, costs, dt, rad, 0, 1, 0.02, horizon, skip, cases.SEP, 0.0, None,
                                             prev, order)
                got = ref.select_pair_clear_tracked(paths, n, live, None, None, None, costs, dt, rad, 0, 1, 0.02, horizon, skip,
                                                    cases.SEP, 0.0, prev, order)
                assert got == want


@pytest.mark.parametrize("shape", ["P2-N5-M3-cap9", "P2-N5-M3-cap70-ragged"])
def test_a_scale_0_term_is_the_path_audit_of_a_sphere_at_rest(oracle, scenes, shape):
    """independent of the term rule's own arithmetic: with scale = 0 the sphere rests at `anchor`, and the term's gap is
    path_audit_reference's clearance of the path against that one obstacle -- the rounding of R and the norm"""
    scs, paths, n, costs, live = oracle_tables(oracle, scenes, shape)
    order = oracle.eval_order()
    rad, dt = scs[0]["radius"], scs[0]["dt"]
    cpl = cases.coupling(shape, "three", scs)
    for p, q, base in ((0, 1, 1), (1, 0, 1 + len(live[0]) - 1)):
        terms = [t for t in ref.terms_of(cpl, 0, 1, live, rad, cases.SEP, None) if t[0] == base + 1]
        assert len(terms) == 1 and terms[0][2] == 0.0
        rest = [float(v) for v in cpl["anchor"][p][1]] + [0.0, 0.0, 0.0, float(live[p][1][6])]
        for i in range(len(n[p])):
            held = [paths[p][i][k] for k in range(int(n[p][i]))]
            want = par.audit_path(held, [rest], dt, rad, 0.0, order)[0]
            for j in range(len(n[q])):
                other = [paths[q][j][k] for k in range(int(n[q][j]))]
                pa, pb = (held, other) if p == 0 else (other, held)
                got = ref.attached_pair(pa, pb, terms, order)
                assert got[0] == want and got[2] == base + 1, (p, i, j, got, want)


@pytest.mark.parametrize("group", list(cases.SHAPE_GROUPS))
def test_every_mutant_changes_an_output_in_every_shape_group(oracle, scenes, group):
    order = oracle.eval_order()
    hit = {m: 0 for m in ref.MUTANTS}
    for shape in cases.SHAPE_GROUPS[group]:
        tables = oracle_tables(oracle, scenes, shape)
        scs, paths, n, costs, live = tables
        for kind in cases.kinds(shape):
            cpl = cases.coupling(shape, kind, scs)
            if cpl is None:
                continue
            tracks = stale_tracks(scs, paths, n, costs, cpl)
            seps = (tie_separation(scs, live),) if kind == "tie" else (cases.SEP,)
            for sep in seps:
                cache = {}
                want = answers(tables, cpl, tracks, order, None, sep, cache)
                seen = 0
                for m in ref.MUTANTS:
                    if answers(tables, cpl, tracks, order, m, sep, cache) != want:
                        hit[m] += 1
                        seen += 1
                print(shape, kind, sep, "mutants seen:", seen)
                assert seen >= 1, (shape, kind)
    assert all(v >= 1 for v in hit.values()), hit


def test_the_tie_goes_to_the_smallest_term(oracle, scenes):
    """scale = 1, anchor = 0 and R = separation: term 1 ties with term 0 in d2 AND in the gap; the code stays 0"""
    shape = "P2-N5-M3-cap9"
    scs, paths, n, costs, live = oracle_tables(oracle, scenes, shape)
    cpl = cases.coupling(shape, "tie", scs)
    sep = tie_separation(scs, live)
    assert live[1][0][6] < live[0][0][6]
    clr, step, sphere = ref.cross_audit_attached(paths[0], n[0], paths[1], n[1], cpl, 0, 1, live, scs[0]["radius"], sep,
                                                 oracle.eval_order())
    base = car.cross_audit(paths[0], n[0], paths[1], n[1], sep, oracle.eval_order())
    zero = [(i, j) for i in range(5) for j in range(5) if sphere[i][j] == 0]
    assert zero, "no pair of this case is decided by the end effectors"
    for i, j in zero:
        assert (clr[i][j], step[i][j]) == (base[0][i][j], base[1][i][j])
    assert all(1 not in row for row in sphere)


# ---- the pre-conditions of the GPU suite's behavioural cases ----
BEHAVIOUR = dict(obstacle_margin=-0.5, pair_margin=0.0, skip_trailing=1)
BEHAVIOUR_SHAPES = ("P2-N5-M3-cap9", "P2-N5-M3-cap70-ragged")


def behaviour_step(n, pair, horizon):
    """a step inside both members' windows, as deep as they go"""
    return min(int(n[0][pair[0]]), int(n[1][pair[1]]), horizon) - 1


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("shape", BEHAVIOUR_SHAPES)
def test_preconditions_of_the_behavioural_gpu_cases(oracle, scenes, shape, side):
    """on the chosen scenes the untracked joint reference returns rule 0 or 1 with a pair (i*, j*); with a sphere of one
    list riding on the other member and sitting on this member's point, its live row far away, the untracked reference
    still returns (i*, j*) and the attached reference another pair or rule 2"""
    scs, paths, n, costs, live = oracle_tables(oracle, scenes, shape)
    order = oracle.eval_order()
    dt, rad, cap = scs[0]["dt"], scs[0]["radius"], scs[0]["max_prediction_steps"]
    b = BEHAVIOUR
    plain = pcr.select_pair_clear(paths, n, live, costs, dt, rad, 0, 1, b["obstacle_margin"], cap, b["skip_trailing"], cases.SEP,
                                  b["pair_margin"], None, None, order)
    assert plain["rule"] in (0, 1) and plain["pair"][0] >= 0, plain
    k = behaviour_step(n, plain["pair"], cap)
    assert k >= 1
    cpl = cases.sphere_on_the_pair(2, len(live[0]) - 1, paths, n, plain["pair"], k, side)
    far = cases.far_rows(live, cpl).tolist()
    again = pcr.select_pair_clear(paths, n, far, costs, dt, rad, 0, 1, b["obstacle_margin"], cap, b["skip_trailing"], cases.SEP,
                                  b["pair_margin"], None, None, order)
    assert again["pair"] == plain["pair"] and again["rule"] == plain["rule"]
    got = ref.select_pair_clear_tracked(paths, n, far, None, None, cpl, costs, dt, rad, 0, 1, b["obstacle_margin"], cap,
                                        b["skip_trailing"], cases.SEP, b["pair_margin"], None, order)
    print(shape, side, "untracked", plain["pair"], plain["rule"], "attached", got["pair"], got["rule"], got["clearance"])
    assert got["pair"] != plain["pair"] or got["rule"] == 2
    assert got["pair"] != plain["pair"], "the pair with the sphere on it must not be returned"


def test_a_stale_track_through_the_path_counts_only_for_a_third_population(oracle, scenes):
    """P = 3: column 0 of arm 0's list rides on arm 1 (S_ab: left out of the obstacle side although its stale track --
    the sphere on arm 0's own selected path -- runs through the paths), column 2 rides on population 2 (stays)"""
    shape = "P3-N5-M3-cap70-ragged"
    scs, paths, n, costs, live = oracle_tables(oracle, scenes, shape)
    order = oracle.eval_order()
    dt, rad, cap = scs[0]["dt"], scs[0]["radius"], scs[0]["max_prediction_steps"]
    cpl = cases.coupling(shape, "one", scs)
    assert ref.attached_columns(cpl, 0, 1) == [0] and ref.attached_columns(cpl, 0, 2) == [2]
    tracks = through_the_paths(scs, paths, n, costs, cpl, 0)
    kept = ref.obstacle_side(paths, n, live, tracks, None, cpl, 0, 1, dt, rad, 0.0, cap, 1, order, mutant="columns_kept")
    left = ref.obstacle_side(paths, n, live, tracks, None, cpl, 0, 1, dt, rad, 0.0, cap, 1, order)
    assert all(fv < w for fv, w in zip(kept[1][0], kept[2][0])), "the stale track was meant to cut every path of arm 0"
    assert any(fv == w for fv, w in zip(left[1][0], left[2][0]))
    # ... and the column that rides on the third population is still audited
    tracks = through_the_paths(scs, paths, n, costs, cpl, 2)
    third = ref.obstacle_side(paths, n, live, tracks, None, cpl, 0, 1, dt, rad, 0.0, cap, 1, order)
    assert all(fv < w for fv, w in zip(third[1][0], third[2][0]))


def through_the_paths(scs, paths, n, costs, cpl, column):
    """stale_tracks with one column of arm 0's list put ON arm 0's own cheapest path: a track that runs through the paths"""
    tracks = stale_tracks(scs, paths, n, costs, cpl)
    best = int(np.argmin(costs[0]))
    t0 = np.asarray(tracks[0])
    for k in range(len(t0)):
        t0[k, column, 0:3] = paths[0][best][min(k, int(n[0][best]) - 1)]
    tracks[0] = t0.tolist()
    return tracks


# ---- the binding table, the header, the resource record ----
def test_binding_table_lists_the_exports(pmaf):
    assert {"pmaf_cross_audit_attached", "pmaf_select_pair_clear_tracked"} <= set(pmaf.planner.SYMBOLS)
    for m in ("cross_audit_attached", "select_pair_clear_tracked"):
        assert callable(getattr(pmaf.PmafPlanner, m))


def test_header_keeps_abi_7_and_declares_the_exports():
    hdr = open(os.path.join(ROOT, "include", "pmaf.h")).read()
    assert "#define PMAF_ABI_VERSION 7" in hdr
    for name in ("pmaf_cross_audit_attached", "pmaf_select_pair_clear_tracked"):
        assert "int %s(pmaf_planner *h" % name in hdr


def test_resource_record_of_the_new_kernels(pmaf, hip_lib):
    """k_cross_audit_attached and k_ft_masked_audit: no scratch, no spills; the attached kernel's LDS is k_cross_audit's"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(pmaf.LIB_PATH)), "resource_usage.txt")).read()
    blocks = {b.splitlines()[0]: b for b in re.split(r"(?=Function Name: )", text) if b.startswith("Function Name:")}
    mine = [b for k, b in blocks.items() if re.search(r"\d+k_(cross_audit_attached|ft_masked_audit)", k)]
    assert len(mine) == 2, sorted(blocks)
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b
        assert re.search(r"VGPRs Spill: 0\b", b) and re.search(r"SGPRs Spill: 0\b", b), b
    lds = lambda b: int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
    plain = [b for k, b in blocks.items() if re.search(r"\d+k_cross_auditE", k)]
    att = [b for k, b in blocks.items() if "k_cross_audit_attached" in k]
    assert len(plain) == 1 and lds(att[0]) == lds(plain[0])
