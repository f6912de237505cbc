"""The rollout's per-obstacle reductions at designed obstacle indices, on the CPU: the oracle (oracle/pmaf_oracle.c,
through orc.OraclePlanner) taken through the layouts of tests/hp_layout.py -- exact ties of the closest obstacle, the
closest obstacle skipped by the circular force, tied nearest others of the latch, term lists of chosen lengths -- and
held to the independent high-precision reference. The same cases run on the kernels in tests/test_hp_layout_gpu.py; here
they are shown to be decidable by the reference alone (0 undecidable samples: a condition on the inputs), each case's
own precondition is re-evaluated in the reference, both sides of the branches concerned are seen, and the cases have
teeth: an oracle handed a falsified obstacle list (the shadow keeps the true one) fails, each mutant on a named case.
Run with -s to see the per-mapping report.

CPU cost, measured on one core with the oracle in the planner's place (the reference costs 1 - 3 ms per obstacle, agent
and step, a latch of an Obstacle / GoalObstacle agent M norms more; hp_layout.cases says which agents are shadowed):
M = 16 .. 64 (one slot, both force sums; group and generic kernels) 8 .. 17 s per mapping, M = 61 .. 128 (two slots, the
split kernel) 4 .. 17 s, M = 183 .. 256 12 .. 33 s, M = 256 on four slots 50 s; the module 6.5 min. K is thinned (named in
hp_layout.family_c); the tie index sets are whole in families A and B, and at M >= 183 their one-step cases alone (13 of
family A, 38 of family B at M = 256, 0.75 s each) are what the time goes to.
"""
import numpy as np
import pytest

import hp_layout as hl
import hp_reference as hp
import hp_shadow as sh

_DONE = {}


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


def _oracle(orc):
    return lambda sc: orc.OraclePlanner(sc, mgr_init_pos=sc["start"])


def _mapping(orc, key):
    """every case of a mapping on the oracle: (cases, Stats)"""
    if key not in _DONE:
        A = hp.Arith("xact")
        st = sh.Stats(key)
        cs = hl.cases(hl.BY_KEY[key])
        for c in cs:
            f0 = len(st.failures)
            hl.run_case(c, _oracle(orc), A, st)
            assert len(st.failures) == f0, (c.name, st.failures[f0:f0 + 4])
        _DONE[key] = (cs, st)
    return _DONE[key]


@pytest.mark.parametrize("key", [m.key for m in hl.MAPPINGS])
def test_designed_layouts(orc, key):
    """every case of families A, B and C for the mapping: within the reference's bound, decided by the reference alone,
    the case's precondition holding in the reference"""
    cs, st = _mapping(orc, key)
    assert {c.family for c in cs} == set(hl.BY_KEY[key].families)
    hl.assert_decided(st, sum(len(c.agents) for c in cs), 1)


def test_layout_branch_coverage(orc):
    """both sides of the branches the layouts are about were decided"""
    seen = {}
    for key in ("w64-one-slot-M60", "grp-16x2", "mw-W3-M100-forced"):
        for k, v in _mapping(orc, key)[1].seen.items():
            seen.setdefault(k, set()).update(v)
    for b in ("scale_closest", "closest_other", "skip_dir", "skip_vel", "shell", "known", "vel_norm", "min_obs"):
        assert seen.get(b) == {True, False}, (b, seen.get(b))


def test_index_sets_sit_where_the_mappings_differ():
    """the tie sets' own claims about lanes, slots and waves, from the recorded mappings"""
    for mp in hl.MAPPINGS:
        sets = hl.tie_sets(mp)
        assert all(len(set(t)) == len(t) and max(t) < mp.M for t in sets), (mp.key, sets)
        if mp.units > 1:
            # a tie whose lower index sits in a higher lane of a lower slot / wave, and one across a unit boundary
            assert any(mp.unit(min(t)) < mp.unit(max(t)) and mp.lane(min(t)) > mp.lane(max(t)) for t in sets), mp.key
            assert any(max(t) - min(t) == 1 and mp.unit(min(t)) != mp.unit(max(t)) for t in sets), mp.key
            assert any(mp.M - 1 in t for t in sets), mp.key
        if mp.kind == "mw" and mp.units >= 3:
            assert any(len({mp.unit(i) for i in t}) == 3 for t in sets), mp.key
        if mp.kind == "mw":
            assert mp.units == mp.waves and mp.per * mp.waves >= mp.M > mp.per * (mp.waves - 1), mp.key


# ---------------------------------------------------------------------------------------------------------------------
# teeth: the oracle handed a falsified obstacle list
# ---------------------------------------------------------------------------------------------------------------------
def _swap(i, j):
    def f(rows):
        rows[[i, j]] = rows[[j, i]]
        return rows
    return f


def _reverse(lo, hi):
    def f(rows):
        rows[lo:hi] = rows[lo:hi][::-1].copy()
        return rows
    return f


def _remove(i):
    def f(rows):
        rows[i] = hl.far_row(i)
        return rows
    return f


def _duplicate(i, at):
    def f(rows):
        rows[at] = rows[i]
        return rows
    return f


def _with_velocity(i, v):
    def f(rows):
        rows[i, 3:6] = v
        return rows
    return f


def _one_ulp_closer(i):
    def f(rows):
        rows[i, 0] = np.nextafter(rows[i, 0], 0.0)
        return rows
    return f


W1, G16, MW3 = hl.W64_ONE, hl.BY_KEY["grp-16x2"], hl.BY_KEY["mw-W3-M100-forced"]
_T17 = hl.term_case(W1, hl._spread(17, 0, 60, 7), "spread")
_H17 = _T17.info["holders"]
_T33 = hl.term_case(G16, hl._spread(32, 0, 32, 1), "all")
_FREE = next(i for i in range(60) if i not in _H17 and i != _T17.info["zero"])
_LATCH = hl.latch_case(MW3, [(MW3.M - 1, hl.ENTER, [(MW3.per, hl.NEIGH[0]), (MW3.per - 1, hl.NEIGH[1])])], False)
_L100 = hl.latch_case(MW3, [(70, hl.ENTER, [])], False, far100=(70, 2), tag=" 100 m")
# mutant -> [(case, falsification, what the reference's failure names)]
MUTANTS = {
    "tied obstacles swapped: the higher index wins": [
        (hl.tie_case(W1, (0, 59)), _swap(0, 59), "path["), (hl.tie_case(G16, (17, 5)), _swap(17, 5), "path["),
        (hl.tie_case(MW3, (MW3.per - 1, MW3.per)), _swap(MW3.per - 1, MW3.per), "path[")],
    "list reversed within one slot / wave range": [
        (hl.tie_case(W1, (0, 59)), _reverse(0, 60), "path["),
        (hl.tie_case(MW3, (MW3.per + 3, MW3.per + 30)), _reverse(MW3.per, 2 * MW3.per), "path[")],
    "term holder removed at list position 0": [(_T17, _remove(_H17[0]), "path[")],
    "term holder removed at list position 15": [(_T17, _remove(_H17[15]), "path[")],
    "term holder removed at list position 16": [(_T17, _remove(_H17[16]), "path[")],
    "term holder removed at the last list position": [(_T33, _remove(31), "path[")],
    "term holder duplicated": [(_T17, _duplicate(_H17[8], _FREE), "path[")],
    "skipped closest obstacle removed: scaling from the wrong obstacle": [
        (hl.skipped_closest_case(W1, 55, 3), _remove(55), "path["),
        (hl.skipped_closest_case(MW3, MW3.M - 1, 0), _remove(MW3.M - 1), "path[")],
    "skipped closest obstacle unskipped: min_obs_dist lowered": [
        (hl.skipped_closest_case(W1, 55, 3), _with_velocity(55, hl.V0), "min_obs_dist["),
        (hl.skipped_closest_case(G16, 23, 3), _with_velocity(23, hl.V0), "min_obs_dist[")],
    "tied neighbour of a latch swapped": [(_LATCH, _swap(MW3.per, MW3.per - 1), "rot[")],
    "100 m neighbour one ulp closer": [(_L100, _one_ulp_closer(2), "rot[")],
}


def test_mutant_cases_pass_unfalsified(orc):
    """the named cases with the true list: nothing flagged (so a mutant's failure is its falsification's)"""
    A = hp.Arith("xact")
    st = sh.Stats("mutant cases, true input")
    n = 0
    for lst in MUTANTS.values():
        for case, _, _ in lst:
            hl.run_case(case, _oracle(orc), A, st)
            n += len(case.agents)
    hl.assert_decided(st, n, 1)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_caught(orc, name):
    """on each named case the independent reference itself flags the falsified input"""
    for case, mutate, what in MUTANTS[name]:
        st = sh.Stats(name)
        hl.run_case(case, _oracle(orc), hp.Arith("xact"), st, mutate=mutate, check_pre=False)
        print(st.report())
        assert any(f.startswith(what) for f in st.failures), (name, case.name, st.failures[:4])
