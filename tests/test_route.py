"""The rollout route (csrc/pmaf_route.hpp): the one pure function that decides which rollout kernel a handle launches and
with what, driven without a library or a device through tests/cpp/route_table.cpp (compiled here, records on stdin /
stdout). Held to
  a. the mappings of tests/hp_layout.py (what the GPU suite asserts of launch_config() case by case),
  b. the dispatch rows of tests/test_zz_perf_guard_gpu.py with the slicing rule as written there,
  c. both sides of every boundary of the rule,
  d. the invariants between the result's fields over the grid of those values crossed,
  e. pmaf_pick_lanes_per_agent, which exports the route's own mapping choice.
The decision has no counterpart in the reference (one std::thread per agent, B/src/cf_manager.cpp:118-123)."""
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest

import conftest
import hp_layout
import test_zz_perf_guard_gpu as guard

ROOT = conftest.ROOT
CSRC = os.path.join(ROOT, "predictive-multi-agent-framework_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

EXTERNAL, MULTI_WAVE, WAVE_PER_AGENT, GROUP, GENERIC = range(5)
IEEE, FAST, XACT, FMA = range(4)
KIND = {"w64": WAVE_PER_AGENT, "mw": MULTI_WAVE, "grp": GROUP, "generic": GENERIC}
IN = ("N", "P", "M", "n_simds", "lanes", "math", "plain", "external", "refused", "force_generic", "mw", "mw_per", "mw_lds_kb",
      "dpp", "slice")
OUT = ("family", "lpa", "slots", "tiles", "waves", "per", "lds_kb", "sliced", "dpp_sum", "plain_out", "math_out", "closest_table",
       "tuned_real_step", "n_blocks", "lds_rollout")
SIMDS = 1024


def rec(N=6, P=1, M=32, n_simds=SIMDS, lanes=0, math=XACT, plain=1, external=0, refused=0, force_generic=0, mw=-1, mw_per=0,
        mw_lds_kb=0, dpp=1, slice=1):
    """an input record; the defaults are a handle created with nothing in the environment"""
    v = locals()
    return tuple(int(v[k]) for k in IN)


def env_rec(env, **kw):
    """the environment as pmaf_create reads it into the record"""
    e = dict(env)
    if "PMAF_FORCE_GENERIC" in e:
        kw["force_generic"] = e.pop("PMAF_FORCE_GENERIC")[:1] == "1"
    if "PMAF_SUM" in e:
        kw["dpp"] = e.pop("PMAF_SUM")[:1] == "d"
    if "PMAF_MW" in e:
        kw["mw"] = int(e.pop("PMAF_MW"))
    assert not e, e
    return rec(**kw)


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "route_table")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                        "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "route_table.cpp"), "-o", exe], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()

    def run(records):
        """records: a sequence of input tuples -> {column: int64 array} of the inputs and the results"""
        a = np.asarray(records, dtype=np.int64).reshape(-1, len(IN))
        fmt = " ".join(["%d"] * len(IN))
        text = "\n".join([fmt % tuple(row) for row in a.tolist()]) + "\n"
        out = subprocess.run([exe], input=text.encode(), capture_output=True, check=True).stdout
        o = np.fromstring(out.decode(), dtype=np.int64, sep=" ").reshape(-1, len(OUT))
        assert len(o) == len(a)
        d = {k: a[:, i] for i, k in enumerate(IN)}
        d.update({k: o[:, i] for i, k in enumerate(OUT)})
        return d

    def one(**kw):
        return {k: int(v[0]) for k, v in run([rec(**kw)]).items()}
    run.one = one
    return run


# ---- a. the designed layouts' mappings --------------------------------------------------------------------------------
@pytest.mark.parametrize("mp", hp_layout.MAPPINGS, ids=lambda m: m.key)
def test_hp_layout_mappings(route, mp):
    r = route([env_rec(mp.env, N=mp.n_agents, M=mp.M, lanes=mp.lpa)])
    assert r["family"][0] == KIND[mp.kind]
    got = dict(lanes_per_agent=r["lpa"][0], waves_per_agent=r["waves"][0], priority_slices=bool(r["sliced"][0]),
               obstacles_per_wave=r["per"][0])
    assert {k: got[k] for k in mp.expect} == mp.expect
    if mp.kind != "mw":
        assert got["obstacles_per_wave"] == mp.M          # what pmaf_get_waves_per_agent reports beside one wave


# ---- b. the perf guards' dispatch rows ----------------------------------------------------------------------------------
def _rows(fn):
    return [m.args[1] for m in fn.pytestmark if m.name == "parametrize"][0]


def test_perf_guard_dispatch_rows(route, scenes):
    shape = {k: (c["n_agents"], 1, c["n_field"]) for k, c in scenes.CONFIGS.items()}
    d = {p.name: p.default for p in inspect.signature(scenes.dual_arm_scenes).parameters.values()}
    shape["C4"] = (d["n_agents"], 2, d["n_field"])
    for cfg, _, _, lpa, waves in guard.BASELINE_CASES:
        N, P, M = shape[cfg]
        r = route.one(N=N, P=P, M=M)
        assert (r["lpa"], r["waves"]) == (lpa, waves), (cfg, r)
    N, _, M = shape["C5"]
    for pops, _, lpa in _rows(guard.test_c5_populations_per_gpu_kernel_time):
        r = route.one(N=N, P=pops, M=M)
        assert (r["lpa"], r["waves"], bool(r["sliced"])) == (lpa, 1, pops == 2), (pops, r)
    for n, m, _, lpa, waves in _rows(guard.test_many_agent_kernel_time):
        r = route.one(N=n, M=m)
        assert (r["lpa"], r["waves"]) == (lpa, waves), (n, m, r)
        assert bool(r["sliced"]) == (lpa == 64 and m <= 60 and 1024 < n <= 2048), (n, m, r)
        assert r["family"] == (MULTI_WAVE if waves > 1 else WAVE_PER_AGENT if lpa == 64 else GROUP), (n, m, r)


# ---- c. the boundaries, each on both sides ------------------------------------------------------------------------------
def test_obstacle_count_boundaries(route):
    want = {   # M: (default: family, waves, per), (PMAF_MW=0: family, slots, TILES, closest_table)
        60: ((WAVE_PER_AGENT, 1, 60), (WAVE_PER_AGENT, 1, 1, 0)), 61: ((MULTI_WAVE, 2, 31), (WAVE_PER_AGENT, 2, 2, 1)),
        64: ((MULTI_WAVE, 2, 32), (WAVE_PER_AGENT, 2, 2, 1)), 65: ((MULTI_WAVE, 2, 33), (WAVE_PER_AGENT, 2, 2, 1)),
        128: ((MULTI_WAVE, 2, 64), (WAVE_PER_AGENT, 2, 2, 1)), 129: ((MULTI_WAVE, 3, 43), (WAVE_PER_AGENT, 3, 4, 1)),
        192: ((MULTI_WAVE, 3, 64), (WAVE_PER_AGENT, 3, 4, 1)), 193: ((MULTI_WAVE, 4, 49), (WAVE_PER_AGENT, 4, 4, 1)),
        256: ((MULTI_WAVE, 4, 64), (WAVE_PER_AGENT, 4, 4, 1)), 257: ((GENERIC, 1, 257), (GENERIC, 5, 0, 0))}
    for M, (dflt, one_wave) in want.items():
        r = route.one(M=M)
        assert (r["family"], r["waves"], r["per"]) == dflt, (M, r)
        r = route.one(M=M, mw=0)
        assert (r["family"], r["slots"], r["tiles"], r["closest_table"]) == one_wave and r["lpa"] == 64, (M, r)
        assert r["lds_rollout"] == 8 * lds_doubles(M, r["tiles"] in (1, 2)), (M, r)


def test_agent_count_boundaries(route):
    for N, P, fam in ((256, 1, MULTI_WAVE), (257, 1, WAVE_PER_AGENT), (128, 2, MULTI_WAVE), (129, 2, WAVE_PER_AGENT)):
        assert route.one(N=N, P=P, M=128)["family"] == fam, (N, P)
    assert route.one(N=128, M=128, n_simds=512)["family"] == MULTI_WAVE        # the CU count is the device's
    assert route.one(N=129, M=128, n_simds=512)["family"] == WAVE_PER_AGENT
    for N, P, sliced in ((1024, 1, 0), (1025, 1, 1), (2048, 1, 1), (2049, 1, 0), (512, 2, 0), (513, 2, 1), (1024, 2, 1), (1025, 2, 0)):
        r = route.one(N=N, P=P, M=32, lanes=64)
        assert (r["family"], r["sliced"]) == (WAVE_PER_AGENT, sliced), (N, P, r)
        assert route.one(N=N, P=P, M=32)["sliced"] == sliced, (N, P)           # ... and with the mapping chosen


def test_multi_wave_switches(route):
    for mw, split in ((-1, (2, 50)), (0, (1, 100)), (2, (2, 50)), (3, (3, 34)), (4, (4, 25)), (5, (2, 50))):
        r = route.one(M=100, mw=mw)
        assert (r["waves"], r["per"]) == split and r["family"] == (WAVE_PER_AGENT if mw == 0 else MULTI_WAVE), (mw, r)
    for mw in (2, 3):                                                            # fewer than the obstacles need: ignored
        r = route.one(M=200, mw=mw)
        assert (r["family"], r["waves"], r["per"]) == (MULTI_WAVE, 4, 50), (mw, r)
    for mw_per, per in ((0, 50), (49, 50), (50, 50), (51, 51), (64, 64), (65, 50)):
        r = route.one(M=100, mw_per=mw_per)
        assert (r["family"], r["waves"], r["per"]) == (MULTI_WAVE, 2, per), (mw_per, r)
    assert route.one(M=100, mw_lds_kb=72)["lds_kb"] == 72 and route.one(M=100, mw=0, mw_lds_kb=72)["lds_kb"] == 0


def test_other_switches(route):
    sl = dict(N=2048, M=32)
    assert route.one(**sl)["sliced"] == 1
    for off in (dict(math=IEEE), dict(math=FAST), dict(dpp=0), dict(slice=0), dict(plain=0), dict(external=1), dict(force_generic=1)):
        r = route.one(**sl, **off)
        assert r["sliced"] == 0, off
        assert r["family"] == (EXTERNAL if "external" in off else GENERIC if "force_generic" in off else WAVE_PER_AGENT), off
    assert route.one(**sl, math=FMA)["sliced"] == 1
    r = route.one(**sl, dpp=0, plain=0)
    assert (r["dpp_sum"], r["plain_out"]) == (0, 0)
    # the compiler-IEEE policy has no multi-wave kernel; every other policy has
    assert [route.one(M=100, math=m)["family"] for m in (IEEE, FAST, XACT, FMA)] == [WAVE_PER_AGENT] + [MULTI_WAVE] * 3
    # an external kernel replaces the launch; the figures the getters report stay
    a, b = route.one(M=100), route.one(M=100, external=1)
    assert b["family"] == EXTERNAL and {k: v for k, v in a.items() if k not in ("family", "external")} == \
        {k: v for k, v in b.items() if k not in ("family", "external")}
    # the policy handed to the launcher: the group kernels have no plain fast arithmetic
    assert [route.one(N=64, M=16, lanes=16, math=m)["math_out"] for m in (IEEE, FAST, XACT, FMA)] == [IEEE, XACT, XACT, FMA]
    assert [route.one(M=16, math=m)["math_out"] for m in (IEEE, FAST, XACT, FMA)] == [IEEE, FAST, XACT, FMA]
    assert [route.one(math=m)["tuned_real_step"] for m in (IEEE, FAST, XACT, FMA)] == [0, 0, 1, 0]
    assert route.one(force_generic=1)["tuned_real_step"] == 0


def test_requested_mappings(route):
    """every power of two, with one and with five obstacle slots per lane"""
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        tuned = lanes >= 8
        r = route.one(lanes=lanes, M=min(lanes, 60))
        fam = WAVE_PER_AGENT if lanes == 64 else GROUP if tuned else GENERIC
        assert (r["family"], r["lpa"], r["slots"], r["tiles"]) == (fam, lanes, 1, 1 if tuned else 0), (lanes, r)
        r = route.one(lanes=lanes, M=5 * lanes)
        assert (r["family"], r["lpa"], r["slots"], r["tiles"]) == (GENERIC, lanes, 5, 0), (lanes, r)
        for s, tiles in ((2, 2), (3, 4), (4, 4)):
            r = route.one(lanes=lanes, M=s * lanes, mw=0)
            assert (r["family"], r["slots"], r["tiles"]) == (fam, s, tiles if tuned else 0), (lanes, s, r)
        assert route.one(lanes=lanes, M=lanes, force_generic=1)["family"] == GENERIC


# ---- d. invariants over the grid ----------------------------------------------------------------------------------------
M_VALUES = (32, 60, 61, 64, 65, 128, 129, 192, 193, 256, 257)
NP_VALUES = ((6, 1), (256, 1), (128, 2), (257, 1), (1024, 1), (1025, 1), (2048, 1), (1024, 2), (2049, 1))
MW_VALUES = (-1, 0, 2, 3, 4)
MW_PER_VALUES = (0, 10, 65)
LANES_ROWS = [rec(N=N, M=M, lanes=lanes, math=math, force_generic=fg) for lanes in (1, 2, 4, 8, 16, 32, 64) for M in (min(lanes, 60), 5 * lanes)
              for N in (6, 2049) for math in range(4) for fg in (0, 1)]


@pytest.fixture(scope="module")
def grid(route):
    b = (0, 1)
    axes = dict(M=M_VALUES, NP=range(len(NP_VALUES)), mw=MW_VALUES, mw_per=MW_PER_VALUES, math=range(4), plain=b, external=b, refused=b,
                force_generic=b, dpp=b, slice=b)
    cross = dict(zip(axes, np.array(list(itertools.product(*axes.values())), dtype=np.int64).T))
    cross["N"], cross["P"] = np.array(NP_VALUES)[cross["NP"]].T
    default = dict(zip(IN, rec()))
    rows = np.stack([cross[k] if k in cross else np.full(len(cross["M"]), default[k]) for k in IN], axis=1)
    return route(np.concatenate([rows, np.array(LANES_ROWS)]))


def lds_doubles(M, two_slot_area):
    """obstacle table (7 per obstacle, the trailing repulsive one included) + known flags (two per double) rounded up to
    even, the list area of pmaf_types.hpp, 32 more"""
    n_obs = M + 1
    flags = (n_obs + 1) // 2
    table = 7 * n_obs + flags
    table += table & 1
    return table + (64 * np.where(two_slot_area, 2, 4) + 8 + 64) * 4 + 32


def test_grid_invariants(grid):
    g = grid
    NP = g["N"] * g["P"]
    assert len(NP) > 300000
    sliced, mw, fam = g["sliced"] == 1, g["family"] == MULTI_WAVE, g["family"]
    assert sliced.sum() >= 100 and all((fam == f).sum() >= 1000 for f in range(5))        # the grid reaches every family
    ok = (fam == WAVE_PER_AGENT) & (g["slots"] == 1) & (g["tiles"] == 1) & (g["dpp_sum"] == 1) & (g["plain_out"] == 1) & \
        ((g["math_out"] == XACT) | (g["math_out"] == FMA)) & (NP > g["n_simds"]) & (NP <= 2 * g["n_simds"])
    assert ok[sliced].all()
    ok = (g["M"] >= 61) & (g["M"] <= 256) & (g["math_out"] != IEEE) & (NP <= g["n_simds"] // 4) & (g["waves"] >= 2) & (g["waves"] <= 4) & \
        (g["waves"] * g["per"] >= g["M"]) & (g["per"] <= 64)
    assert ok[mw].all()
    assert ((g["waves"] == 1) & (g["per"] == g["M"]))[(g["waves"] < 2)].all() and (g["waves"] >= 1).all()
    assert (g["waves"] == 1)[(fam != MULTI_WAVE) & (fam != EXTERNAL)].all()
    assert ((g["closest_table"] == 1) == ((g["lpa"] == 64) & (g["M"] >= 61) & (g["M"] <= 256) & (g["force_generic"] == 0))).all()
    assert (g["n_blocks"] == (g["N"] * g["lpa"] + 63) // 64).all()
    # the LDS request follows the routed kernel: the two-slot list area exactly when it is a tuned kernel with one or two
    # obstacle slots per lane (TILES 1 / 2) -- from the inputs: a tuned mapping, not forced generic, and at most two slots needed
    two = (g["tiles"] == 1) | (g["tiles"] == 2)
    tuned = np.isin(g["lpa"], (8, 16, 32, 64)) & (g["force_generic"] == 0)
    need = np.where(g["lpa"] == 64, np.where(g["M"] <= 60, 1, np.where(g["M"] <= 64, 2, (g["M"] + 63) // 64)), (g["M"] + g["lpa"] - 1) // g["lpa"])
    assert (two == (tuned & (need <= 2))).all()
    assert ((g["tiles"] == 4) == (tuned & (need >= 3) & (need <= 4))).all() and ((g["tiles"] == 0) == ~(tuned & (need <= 4))).all()
    assert (g["slots"] == np.where(g["tiles"] > 0, need, (g["M"] + g["lpa"] - 1) // g["lpa"])).all()
    assert (g["lds_rollout"] == 8 * lds_doubles(g["M"], two)).all()
    # families: forced generic and untuned shapes run the generic kernel; the figures pass through
    assert (fam == EXTERNAL)[g["external"] == 1].all() and (fam != EXTERNAL)[g["external"] == 0].all()
    assert (fam == GENERIC)[(g["tiles"] == 0) & (g["external"] == 0)].all()
    assert (g["tuned_real_step"] == ((g["math"] == XACT) & (g["force_generic"] == 0))).all()
    assert (g["dpp_sum"] == g["dpp"]).all() and (g["plain_out"] == g["plain"]).all()
    grp = (g["tiles"] > 0) & (g["lpa"] < 64)                     # (under an external kernel too: the figures pass through)
    assert (fam == GROUP)[grp & (g["external"] == 0)].all()
    assert (g["math_out"] == np.where(grp & (g["math"] == FAST), XACT, g["math"])).all()


def test_refusal_routes_like_pmaf_mw_0(grid, route):
    """a handle the multi-wave launcher refused gets what PMAF_MW=0 gives, whatever else is set"""
    g = grid
    idx = np.nonzero(g["refused"] == 1)[0][::5]
    assert len(idx) > 30000 and (g["family"][np.nonzero(g["refused"] == 0)[0]] == MULTI_WAVE).any()
    twin = np.stack([np.zeros(len(idx), dtype=np.int64) if k in ("mw", "refused") else g[k][idx] for k in IN], axis=1)
    t = route(twin)
    for k in OUT:
        assert (t[k] == g[k][idx]).all(), k
    assert (g["family"][idx] != MULTI_WAVE).all() and (g["waves"][idx] == 1).all()


# ---- e. the exported mapping choice ----------------------------------------------------------------------------------
def test_pick_lanes_per_agent_is_the_routes_choice(grid, hip_lib, route):
    g = grid
    shapes = sorted({(int(n), int(p), int(m)) for n, p, m, l, s in zip(g["N"], g["P"], g["M"], g["lanes"], g["n_simds"]) if l == 0 and s == SIMDS})
    shapes += [(n, p, m) for n, p, m, _ in ((2304, 1, 9, 16), (2048, 1, 62, 32), (1024, 8, 32, 16), (1024, 4, 32, 32), (8192, 1, 32, 16))]
    r = route([rec(N=n, P=p, M=m) for n, p, m in shapes])
    assert len(shapes) >= len(M_VALUES) * len(NP_VALUES) and len(set(r["lpa"].tolist())) >= 3
    for (n, p, m), lpa in zip(shapes, r["lpa"].tolist()):
        assert hip_lib.pmaf_pick_lanes_per_agent(n, p, m, SIMDS) == lpa, (n, p, m)
