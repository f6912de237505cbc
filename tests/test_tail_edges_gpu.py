"""Edges of the step's closing sqrt / reciprocal / divide sequence and of the obstacle advance, device against the
oracle at tolerance 0 (portable-exp mode, as tests/test_parity_gpu.py): paths, n_points, rotation vectors, known flags
and costs, over three ticks of a small population -- 7 agents (every heuristic), 12 path points.

The closing sequence divides by a lane's norm or by a selected 1.0, and its riders divide vel_max by a norm that may be
zero; every rollout family has one, so one shape per family: the one-slot wave-per-agent kernel (3 field obstacles),
the two-slot one (62, PMAF_MW=0), the multi-wave kernel (65) and the group kernel (16 lanes per agent, 3 obstacles).
Each runs
  * from rest: the first tick starts with zero velocity (the speed clamp's lane divides by a small or zero norm),
  * with k_attr = 0: attractorForce's desired velocity is the zero vector, its rider divides vel_max by a zero norm,
  * with a field obstacle centred on the start position: ro = 0, the lane's divisor is the selected 1.0,
  * with the repulsive obstacle in range from the first step: the lane-60 rider / sentinel_repel_m's direction.
Three obstacles sit within the detection shell of the start, and the attractor is stiff enough (k_attr 10, k_damp 40:
half of vel_max after two steps) for the gate of the circular field to open within the 11 steps of a rollout. The
obstacle on the start position drives an agent's state to NaN once the gate is open -- the reference divides 0 / 0
there -- so that case compares NaN for NaN and everything else bit for bit.

The one-slot kernel's bodies for field obstacles at rest carry no obstacle advance when no coordinate is -0.0 and
0 <= dt < inf (field_obstacles_at_rest, csrc/pmaf_rollout_w64.hpp): an at-rest scene with a +0.0 coordinate (the body
without the advance), the same scene with that coordinate -0.0 -- the agent's own y is exactly 0.0 at the start, so the
sign of ro's zero is live in the first step and the reference's `pos += vel * dt` turns the coordinate into +0.0 behind
it: the bodies that advance --, and moving obstacles, each with the repulsive obstacle out of range and in range."""
import numpy as np
import pytest

from conftest import drive
from test_parity_gpu import make_pair, run_both

pytestmark = pytest.mark.gpu

N_AGENTS, CAP = 7, 12
# name: (field obstacles, lanes_per_agent request, PMAF_MW, (lanes, waves) the handle must report)
SHAPES = {
    "one_slot": (3, 64, None, (64, 1)),
    "two_slot": (62, 64, "0", (64, 1)),
    "multi_wave": (65, 64, None, (64, 2)),
    "group": (3, 16, None, (16, 1)),
}
NEAR = np.array([[-0.45, 0.0, 0.75], [-0.5, 0.12, 0.6], [-0.42, -0.1, 0.68]])   # within 0.35 m of the start (-0.6, 0, 0.7)
IN_RANGE = [-0.45, 0.05, 0.72, 0.0, 0.0, 0.0, 0.05]       # the repulsive obstacle 0.16 m from the start: in range at once


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


def _scene(scenes, m, seed, dynamic=False):
    sc = scenes.synthetic_scene(N_AGENTS, CAP - 1, m, 9, seed, dynamic=dynamic)
    assert sorted(set(sc.get("agent_types", scenes.default_agent_types(N_AGENTS)))) == [1, 2, 3, 4, 5, 6]
    sc["obstacles"][:3, :3] = NEAR
    sc["obstacles"][:3, 6] = 0.04
    sc["k_attr"], sc["k_damp"] = 10.0, 40.0
    return sc


def _same(a, b):
    """bit for bit, any NaN for any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(b)
    np.testing.assert_array_equal(np.isnan(a), nan)
    np.testing.assert_array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def _run(pmaf, oracle, scenes, sc, shape, monkeypatch, dynamic=False, finite=True):
    m, lpa, mw, want = SHAPES[shape]
    if mw is not None:
        monkeypatch.setenv("PMAF_MW", mw)
    if finite:
        hip, ora = run_both(pmaf, oracle, scenes, sc, 3, dynamic=dynamic, lanes_per_agent=lpa)
    else:
        hip, ora = make_pair(pmaf, oracle, sc, lanes_per_agent=lpa)
        bh, _ = drive(hip, sc, 2)
        bo, _ = drive(ora, sc, 2)
        hip.stop()
        np.testing.assert_array_equal(bh, bo)
        assert np.isnan(ora.paths()[0]).any()
    cfg = hip.launch_config()
    assert (cfg["lanes_per_agent"], cfg["waves_per_agent"]) == want, cfg
    (ph, nh), (po, no) = hip.paths(), ora.paths()
    np.testing.assert_array_equal(nh, no)
    for a in range(N_AGENTS):
        _same(ph[a, :no[a]], po[a, :no[a]])
    _same(hip.rot_vecs(), ora.rot_vecs())                  # signs of zeros included
    _same(hip.costs(), ora.costs())
    np.testing.assert_array_equal(hip.known(), ora.known())
    known = hip.known().sum()
    hip.close()
    return known


@pytest.mark.parametrize("case", ["from_rest", "k_attr_zero", "obstacle_on_the_start", "repulsive_in_range"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_tail_edges_in_every_rollout_family(pmaf, oracle, scenes, monkeypatch, shape, case):
    sc = _scene(scenes, SHAPES[shape][0], 40 + len(shape))
    if case == "k_attr_zero":
        sc["k_attr"] = 0.0
    elif case == "obstacle_on_the_start":
        sc["obstacles"][0, :3] = sc["start"]
    elif case == "repulsive_in_range":
        sc["obstacles"][-1] = IN_RANGE
    known = _run(pmaf, oracle, scenes, sc, shape, monkeypatch, finite=(case != "obstacle_on_the_start"))
    assert known > 0 or case == "k_attr_zero"     # some obstacle was latched: the circular field was live


@pytest.mark.parametrize("repulsive", ["far", "in_range"])
@pytest.mark.parametrize("case", ["plus_zero", "minus_zero", "moving"])
def test_obstacle_advance_of_the_one_slot_bodies(pmaf, oracle, scenes, monkeypatch, case, repulsive):
    sc = _scene(scenes, 3, 77, dynamic=(case == "moving"))
    assert sc["start"][1] == 0.0 and not np.signbit(sc["start"][1])
    if case != "moving":
        assert not sc["obstacles"][:3, 3:6].any() and not np.signbit(sc["obstacles"][:3, 3:6]).any()
        sc["obstacles"][0, 1] = 0.0 if case == "plus_zero" else -0.0
        assert np.signbit(sc["obstacles"][0, 1]) == (case == "minus_zero")
    else:
        sc["obstacles"][0, 1] = 0.0
        assert sc["obstacles"][:3, 3:6].all()
    if repulsive == "in_range":
        sc["obstacles"][-1] = IN_RANGE
    assert _run(pmaf, oracle, scenes, sc, "one_slot", monkeypatch, dynamic=(case == "moving")) > 0
