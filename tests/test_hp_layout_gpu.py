"""The rollout kernels' per-obstacle reductions at designed obstacle indices: the layouts of tests/hp_layout.py through
the HIP planner, one test per planner family and obstacle count, every case held to the independent high-precision
reference (tests/hp_reference.py) with 0 undecidable samples. launch_config() is asserted for every case, so each one
is known to have run the mapping it was designed for. Strict policy throughout (exact ties are a strict-policy
property); the term-list cases (family C) also run under the contracted policy.

The nearest other obstacle of the latch (family B) is answered by two code paths, and nothing in the C-ABI reports
which one ran, so it follows from the inputs: with every field obstacle at rest, k_manager writes the closest-other table
at the reset that carries the new list (pmaf_host.cpp: closest_dirty; pmaf_route.hpp: closest_table; pmaf_k_misc.hip: closest_ok =
1 only if no velocity component is non-zero), and k_rollout_w64 with 2 .. 4 slots and k_rollout_mw read it; with one far
obstacle moving, closest_ok = 0 and the same kernels run their cooperative scans. The one-slot kernel, k_rollout_grp and
the generic kernel always scan. Every case is run both ways.

CPU cost of the shadowing, per mapping and family, is in tests/test_hp_layout.py's docstring; it dominates the wall
time here. The module's wall time on the GPU has not been measured yet.
"""
import numpy as np
import pytest
import torch

import hp_layout as hl
import hp_reference as hp
import hp_shadow as sh

pytestmark = pytest.mark.gpu

POLICY_KW = {"xact": {}, "fma": {"contracted": True}}


def _make(pmaf, mp, policy):
    def make(sc):
        pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"], lanes_per_agent=mp.lpa, **POLICY_KW[policy])
        cfg = pl.launch_config()
        for k, v in mp.expect.items():
            if cfg[k] != v:
                pl.close()
                raise AssertionError((mp.key, k, v, cfg))
        return pl
    return make


def _run(pmaf, monkeypatch, mp, cs):
    for k, v in mp.env.items():
        monkeypatch.setenv(k, v)
    st = sh.Stats(mp.key + " [xact]")
    A = hp.Arith("xact")
    for c in cs:
        f0 = len(st.failures)
        hl.run_case(c, _make(pmaf, mp, "xact"), A, st)
        assert len(st.failures) == f0, (c.name, st.failures[f0:f0 + 4])
    hl.assert_decided(st, sum(len(c.agents) for c in cs), 1)
    tc = [c for c in cs if c.family == "C"]
    sf = sh.Stats(mp.key + " [fma]")
    Af = hp.Arith("fma")
    for c in tc:
        f0 = len(sf.failures)
        hl.run_case(c, _make(pmaf, mp, "fma"), Af, sf)
        assert len(sf.failures) == f0, (c.name, sf.failures[f0:f0 + 4])
    hl.assert_decided(sf, sum(len(c.agents) for c in tc), 1)


@pytest.mark.parametrize("key", [m.key for m in hl.MAPPINGS])
def test_designed_layouts(pmaf, monkeypatch, key):
    mp = hl.BY_KEY[key]
    _run(pmaf, monkeypatch, mp, hl.cases(mp))


def test_designed_layouts_sliced(pmaf, monkeypatch):
    """k_rollout_w64_sliced needs more than one wave per SIMD of agents: one tie case and one term-list case at that
    size, the six designed agents shadowed"""
    simds = torch.cuda.get_device_properties(0).multi_processor_count * 4
    mp = hl.Mapping("w64-sliced-M60", 60, "w64", lpa=64, n_agents=simds + simds // 2, sliced=True)
    cs = [hl.tie_case(mp, (59, 0)), hl.term_case(mp, hl._spread(17, 0, 60, 7), "spread")]
    for c in cs:
        c.agents = list(range(6))
    _run(pmaf, monkeypatch, mp, cs)
