"""tests/variant_matrix.py without a device:
  a. every row routes (csrc/pmaf_route.hpp, driven through tests/cpp/route_ftrack_table.cpp) to the instantiation it
     names -- launch_config() reports neither the policy nor the step nor the sum, so this is what ties a row of
     tests/test_variant_matrix_gpu.py to a kernel body;
  b. long_loop_scenes.build_scene's larger populations keep agents 0 ... 6 and the obstacles of the default call;
  c. the bounded legs' condition: with the oracle in the planner's place, tick 0 of every bounded case has 0 undecidable
     samples under the fast and the contracted policy's bound (so what the GPU leaves undecided is the kernels' last
     bits, not the scene);
  d. teeth, under the contracted policy's bound (four times the strict one): an oracle handed a list without the obstacle
     that holds the 17th term, or with one more obstacle inside the shell at the K = 3 step behind K = 25, fails on a path
     point while the shadow keeps the true list.
CPU cost on one core, oracle as planner: 3.4 ... 5.5 s per shadowed tick of seven agents (the reference's rollouts are
shared between the two policies, whose bounds have the same parameters, and between the cases of c. and d.)."""
import os
import subprocess

import numpy as np
import pytest

import conftest
import long_loop_scenes as lls
import sum_chunk_scenes as scs
import test_route as tr
import variant_matrix as vm

ROOT = conftest.ROOT
SIMDS = 1024


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


# ---- a. the rows name the instantiation they claim ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def route(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vm_route") / "route_ftrack_table")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(tr.ROCM, "include"),
                        "-I" + tr.CSRC, os.path.join(ROOT, "tests", "cpp", "route_ftrack_table.cpp"), "-o", exe], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    cols = tr.OUT + ("carries_track", "carries_field_tracks")

    def one(tracked, ftracked, **kw):
        text = "%d %d " % (tracked, ftracked) + " ".join("%d" % v for v in tr.rec(**kw)) + "\n"
        out = subprocess.run([exe], input=text.encode(), capture_output=True, check=True).stdout.split()
        assert len(out) == len(cols)
        return dict(zip(cols, (int(v) for v in out)))
    return one


def _row_scenes(scenes, row):
    """a scene of every kind the row is run on (the route reads N, M, the mass and the gains)"""
    n = vm.crowded_agents(SIMDS) if row.crowded else lls.N_AGENTS
    out = [lls.build_scene(scenes, "runs", False, False, n_agents=n)]
    if not row.crowded:
        out.append(scs.build_scene(scenes, 17, True, True))
    return out


def test_the_matrix_is_the_issues():
    assert [len(g) for g in (vm.STRICT, vm.TRACK, vm.FTRACK, vm.BOUNDED, vm.SLICED)] == [7, 3, 3, 8, 1]
    assert len({r.name for r in vm.ROWS + vm.GENERAL_BY_INPUT}) == len(vm.ROWS) + 4
    inst = [tuple(sorted(r.inst.items())) for r in vm.ROWS]
    assert len(set(inst)) == len(inst) == 22                  # 22 instantiations beside the 4 the default handles run
    default = dict(family=vm.WAVE_PER_AGENT, slots=1, dpp_sum=True, plain=True, math=vm.MATH["xact"], sliced=False)
    assert not any(r.inst == dict(default, kernel=k) for r in vm.ROWS for k in ("w64", "track", "ftrack"))
    assert not any(r.inst == dict(default, kernel="sliced", sliced=True) for r in vm.ROWS)


def test_the_matrix_module_imports_neither_the_oracle_nor_the_package():
    import ast
    tree = ast.parse(open(vm.__file__).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add(node.module or "")
    assert mods <= {"collections", "numpy", "hp_reference", "hp_shadow"}, mods


@pytest.mark.parametrize("row", vm.ROWS, ids=lambda r: r.name)
def test_row_routes_to_its_instantiation(route, scenes, row):
    for sc in _row_scenes(scenes, row):
        assert sc["obstacles"].shape[0] - 1 == 60
        r = route(row.track, row.ftrack, N=sc["n_agents"], M=60, n_simds=SIMDS, math=vm.MATH[row.policy],
                  plain=vm.plain_input(row, sc), dpp=vm.dpp_input(row), lanes=64 if row.crowded else 0)
        got = dict(family=r["family"], slots=r["slots"], dpp_sum=bool(r["dpp_sum"]), plain=bool(r["plain_out"]),
                   math=r["math_out"], sliced=bool(r["sliced"]))
        assert got == {k: v for k, v in row.inst.items() if k != "kernel"}, (row.name, sc["name"], r)
        assert (r["lpa"], r["tiles"], r["waves"]) == (64, 1, 1), r
        if row.track or row.ftrack:
            assert r["carries_track"] == 1 and r["carries_field_tracks"] == 1, r
        assert (row.inst["kernel"] == "sliced") == bool(r["sliced"]) == row.crowded
        assert {"w64": (False, False), "sliced": (False, False), "track": (True, False), "ftrack": (False, True)}[row.inst["kernel"]] == \
            (row.track, row.ftrack)


@pytest.mark.parametrize("row", vm.GENERAL_BY_INPUT, ids=lambda r: r.name)
def test_inputs_that_need_the_general_step_route_to_it(route, scenes, row):
    assert "PMAF_PLAIN_STEP" not in row.env
    base = scs.build_scene(scenes, 17, False, False)
    assert vm.plain_input(row, base)
    for variant in vm.GENERAL_VARIANTS:
        sc = vm.general_scene(base, variant)
        assert not vm.plain_input(row, sc)
        r = route(0, 0, N=sc["n_agents"], M=60, n_simds=SIMDS, math=vm.MATH[row.policy], plain=vm.plain_input(row, sc),
                  dpp=vm.dpp_input(row))
        got = dict(family=r["family"], slots=r["slots"], dpp_sum=bool(r["dpp_sum"]), plain=bool(r["plain_out"]),
                   math=r["math_out"], sliced=bool(r["sliced"]))
        assert got == {k: v for k, v in row.inst.items() if k != "kernel"} and not got["plain"], (row.name, variant, r)
        assert (r["lpa"], r["tiles"]) == (64, 1), r
    sc = vm.general_scene(base, "mass_noattr")
    assert sc["agent_mass"] == 2.5 and [i for i in range(7) if sc["k_attr"][i] == 0.0] == [1, 4]
    assert base["agent_mass"] == 1.0 and np.ndim(base["k_attr"]) == 0      # (the base scene is not modified)


# ---- b. the larger populations of long_loop_scenes ----------------------------------------------------------------------
@pytest.mark.parametrize("name,moving,sent_near", vm.SLICED_LONG_LOOP)
def test_a_larger_population_keeps_the_seven_agents(scenes, name, moving, sent_near):
    d = lls.build_scene(scenes, name, moving, sent_near)
    assert d["n_agents"] == 7 and d["random_vecs"].shape == (7, lls.M + 1, 3)
    np.testing.assert_array_equal(d["agent_types"], scenes.default_agent_types(7))
    assert d["agent_types"].dtype == scenes.default_agent_types(7).dtype
    n = vm.crowded_agents(SIMDS)
    p = lls.build_scene(scenes, name, moving, sent_near, n_agents=n)
    assert p["n_agents"] == n == 1536 and p["random_vecs"].shape == (n, lls.M + 1, 3) and p["agent_types"].shape == (n,)
    np.testing.assert_array_equal(p["random_vecs"][:7], d["random_vecs"])
    np.testing.assert_array_equal(p["agent_types"], np.resize(d["agent_types"], n))
    np.testing.assert_allclose(np.linalg.norm(p["random_vecs"], axis=-1), 1.0, rtol=0, atol=1e-15)
    assert len({v.tobytes() for v in p["random_vecs"][:, 0]}) == n            # (no agent repeats another's vectors)
    for k in d:
        if k not in ("random_vecs", "agent_types", "n_agents"):
            np.testing.assert_array_equal(np.asarray(p[k]), np.asarray(d[k]), err_msg=k)


# ---- c. every bounded case is decided by the reference alone ------------------------------------------------------------
def _oracle_tick(oracle, sc, mod, policy, tag, agents=None, wrap=None):
    pl = oracle.OraclePlanner(sc, mgr_init_pos=mod.INIT)
    try:
        return vm.shadow_first_tick(pl if wrap is None else wrap(pl), sc, mod.INIT, mod.START, policy, tag, agents=agents)
    finally:
        pl.close()


def _assert_decided(st, n_rollouts):
    print(st.report())
    assert not st.failures, st.failures[:4]
    assert st.undecidable == 0, st.report()
    # costs of the sampled agents, the real step and the rollouts; the selection where every agent is sampled
    assert st.rollouts_compared == n_rollouts and st.compared >= 2 * n_rollouts + 1, st.report()


@pytest.mark.parametrize("policy", ["fast", "fma"])
@pytest.mark.parametrize("name,moving,sent_near", vm.BOUNDED_LONG_LOOP)
def test_long_loop_cases_are_decided(oracle, scenes, name, moving, sent_near, policy):
    sc = lls.build_scene(scenes, name, moving, sent_near)
    _assert_decided(_oracle_tick(oracle, sc, lls, policy, sc["name"]), 7)


@pytest.mark.parametrize("policy", ["fast", "fma"])
@pytest.mark.parametrize("K,moving,sent_near", vm.BOUNDED_SUM_CHUNK)
def test_sum_chunk_cases_are_decided(oracle, scenes, K, moving, sent_near, policy):
    sc = scs.build_scene(scenes, K, moving, sent_near)
    _assert_decided(_oracle_tick(oracle, sc, scs, policy, sc["name"]), 7)


@pytest.mark.parametrize("name,moving,sent_near", vm.SLICED_LONG_LOOP)
def test_crowded_cases_are_decided(oracle, scenes, name, moving, sent_near):
    """the sliced row's population of 1.5 x SIMDs agents, agents 0 ... 6 shadowed"""
    sc = lls.build_scene(scenes, name, moving, sent_near, n_agents=vm.crowded_agents(SIMDS))
    _assert_decided(_oracle_tick(oracle, sc, lls, "fma", sc["name"] + " x %d" % sc["n_agents"], agents=range(7)), 7)


# ---- d. teeth -----------------------------------------------------------------------------------------------------------
class _Falsified:
    """a planner whose tick is handed mutate(rows) while the shadow keeps the true rows"""

    def __init__(self, inner, mutate):
        self.inner, self.mutate = inner, mutate

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def tick(self, obs, *a):
        return self.inner.tick(self.mutate(np.array(obs, dtype=np.float64, copy=True)), *a)


def _lattice_terms(sc, j):
    """the holders of a term at lattice point j of a long_loop scene, in list order"""
    return scs.terms_at(sc, [lls.lattice(j), lls.START[1], lls.START[2]], [lls.VMAX, 0.0, 0.0], lls.INIT)


def _mutant_fails(oracle, sc, mod, mutate, tag):
    ok = _oracle_tick(oracle, sc, mod, "fma", tag + ", true list")
    _assert_decided(ok, 7)
    st = _oracle_tick(oracle, sc, mod, "fma", tag, wrap=lambda pl: _Falsified(pl, mutate))
    print(st.report())
    assert st.failures, "the bound swallowed the mutant (k_circ too small for this purpose?):\n" + st.report()
    assert any(f.startswith("path[") for f in st.failures), st.failures[:4]
    return st


def test_mutant_dropped_17th_term_long_loop(oracle, scenes):
    """"runs", step 3 of tick 0 (K = 25, the first long step): the holder of list position 16 is 60 m off in the list the
    oracle gets"""
    sc = lls.build_scene(scenes, "runs", False, True)
    terms = _lattice_terms(sc, 3)
    assert len(terms) == 25 == lls.k_at("runs", 3)
    drop = terms[16]

    def mutate(rows):
        rows[drop, 1] += 60.0
        return rows
    assert len(_lattice_terms(dict(sc, obstacles=mutate(sc["obstacles"].copy())), 3)) == 24
    st = _mutant_fails(oracle, sc, lls, mutate, "runs without the 17th term")
    # the first point it can show at is the one behind step 3
    assert not any(f.startswith("path[%d][%d]" % (a, k)) for f in st.failures for a in range(7) for k in (1, 2, 3)), st.failures[:4]


def test_mutant_dropped_17th_term_sum_chunks(oracle, scenes):
    sc = scs.build_scene(scenes, 17, True, True)
    drop = scs.holders(17)[16]

    def mutate(rows):
        rows[drop, 0:3] = scs.START + 3.0 * (rows[drop, 0:3] - scs.START)
        return rows
    at = dict(sc, obstacles=mutate(sc["obstacles"].copy()))
    assert scs.terms_at(at, scs.START, [0.1, 0.0, 0.0], scs.INIT) == scs.holders(17)[:16]
    _mutant_fails(oracle, sc, scs, mutate, "K = 17 without the 17th term")


def test_mutant_stale_term_behind_the_long_run(oracle, scenes):
    """"runs", step 5 of tick 0 (K = 3 right behind K = 25): the oracle's list has a fourth obstacle in the shell there,
    a far one moved onto the K = 3 cluster's ring -- what a stale second chunk would add"""
    sc = lls.build_scene(scenes, "runs", False, True)
    three = _lattice_terms(sc, 5)
    assert len(three) == 3 == lls.k_at("runs", 5) and lls.k_at("runs", 4) == 25
    far = next(i for i in range(lls.M) if sc["obstacles"][i, 1] >= 60.0)
    src = sc["obstacles"][three[0]]
    y, z = src[1] - lls.START[1], src[2] - lls.START[2]

    def mutate(rows):
        rows[far] = src
        rows[far, 1] = lls.START[1] + np.cos(1.0) * y - np.sin(1.0) * z       # the same ring, one radian on
        rows[far, 2] = lls.START[2] + np.sin(1.0) * y + np.cos(1.0) * z
        return rows
    at = dict(sc, obstacles=mutate(sc["obstacles"].copy()))
    assert [len(_lattice_terms(at, j)) for j in (3, 4, 5, 6)] == [25, 25, 4, 4]
    st = _mutant_fails(oracle, sc, lls, mutate, "runs with a stale term at K = 3")
    assert not any(f.startswith("path[%d][%d]" % (a, k)) for f in st.failures for a in range(7) for k in range(1, 6)), st.failures[:4]
