"""The obstacle tracks (include/pmaf.h "obstacle tracks") without a device: the composed reference of
tests/field_track_reference.py is validated against the oracle's own rollout, every shape group the GPU suite runs
(tests/test_field_track_gpu.py) is shown to be sensitive to each rule of the contract, and the new kernels' resource
record is held to no scratch."""
import os
import re

import numpy as np
import pytest

import field_track_reference as fref
import sentinel_track_reference as sref


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


def fresh(oracle, sc):
    ora = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
    ora.set_initial_position(sc["start"])
    return ora


def untracked(oracle, sc):
    ora = fresh(oracle, sc)
    ora.rollout()
    paths, n = ora.paths()
    out = dict(paths=paths, n_points=n, min_obs=ora.min_obs_dist(), known=ora.known(), rot=ora.rot_vecs(), vel=ora.agent_vel(),
               reached=ora.success())
    ora.evaluate(sc["cost_gains"], sc["ws_limits"])
    out["costs"] = ora.costs()
    return out


def composed(oracle, sc, ftracks, first=0, track=None, mutant=None):
    ora = fresh(oracle, sc)
    out = fref.compose(ora, oracle.eval_order(), sc, sc["obstacles"], ftracks, first, track, mutant)
    ora.evaluate(sc["cost_gains"], sc["ws_limits"])
    out["costs"] = ora.costs()
    return out


def same(a, b, keys=("paths", "n_points", "min_obs", "known", "rot", "vel", "reached", "costs")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("shape", list(fref.SHAPES))
def test_composer_is_the_oracles_rollout(oracle, scenes, shape):
    """no tracks, and the straight lines with the constant velocities as tracks (cap points, one point short of the
    rollout's reads from offset 1 with the first point doubled, and together with the straight-line repulsive track):
    the composer gives orc_rollout's bits"""
    sc = fref.build_scene(scenes, shape)
    want = untracked(oracle, sc)
    assert (want["n_points"] > 1).all()
    cap = sc["max_prediction_steps"]
    same(composed(oracle, sc, None), want)
    lines = fref.straight_lines(sc["obstacles"], sc["dt"], cap)
    same(composed(oracle, sc, lines), want)
    same(composed(oracle, sc, np.concatenate([lines[:1], lines]), first=1), want)
    same(composed(oracle, sc, lines, track=sref.straight_line(sc["obstacles"], sc["dt"], cap)), want)


def _case_tracks(oracle, scenes, shape, _cache={}):
    if shape not in _cache:
        sc = fref.build_scene(scenes, shape)
        un = untracked(oracle, sc)
        _cache[shape] = (sc, un, fref.tracks_for(sc, un["paths"][0], int(un["n_points"][0])))
    return _cache[shape]


@pytest.mark.parametrize("group", list(fref.SHAPE_GROUPS))
def test_cases_are_sensitive(oracle, scenes, group):
    """every mutant of the contract changes path bits in at least one case of every shape group, and every case sees at
    least one of them and differs from the untracked rollout"""
    cases = [c for c in fref.case_list() if c[0] in fref.SHAPE_GROUPS[group]]
    hit = {m: 0 for m in fref.MUTANTS}
    for shape, tname, first in cases:
        sc, un, tracks = _case_tracks(oracle, scenes, shape)
        t = tracks[tname]
        f = fref.resolve_first(first, len(t))
        want = composed(oracle, sc, t, f)
        assert not np.array_equal(want["paths"], un["paths"]), (shape, tname, first)
        seen = 0
        for m in fref.MUTANTS:
            got = composed(oracle, sc, t, f, mutant=m)
            if not (np.array_equal(got["paths"], want["paths"]) and np.array_equal(got["n_points"], want["n_points"])):
                hit[m] += 1
                seen += 1
        assert seen >= 1, (shape, tname, first)
    assert all(v >= 1 for v in hit.values()), hit


@pytest.mark.parametrize("shape", ["M3-cap70", "M59-cap70", "M60-cap70", "M3-cap70-general"])
def test_sweep_latches_on_a_tracked_position(oracle, scenes, shape):
    """the sweeping obstacle is outside every agent's shell at the start, inside it mid-rollout -- where it is latched:
    its known flag is set by the tracked rollout and not by the untracked one -- and outside again at the end"""
    sc, un, tracks = _case_tracks(oracle, scenes, shape)
    t = tracks["sweep"]
    got = composed(oracle, sc, t)
    r0 = sc["obstacles"][0, 6]
    for i in range(fref.N_AGENTS):
        n = int(got["n_points"][i])
        d = [fref.shell_distance(sc, got["paths"][i, k], t[min(k, len(t) - 1), 0, 0:3], r0) for k in range(n - 1)]
        assert d[0] > sc["detect_shell_rad"] and d[-1] > sc["detect_shell_rad"] and min(d) < sc["detect_shell_rad"], (shape, i)
        assert got["known"][i, 0] == 1, (shape, i)
    # on its live-list line the obstacle never comes that close to every agent
    assert not (np.asarray(un["known"])[:, 0] == 1).all()


def test_closed_loop_ticks_depend_on_the_offset(oracle, scenes):
    """the tick sequence the GPU suite runs: every tick's rollout differs from the one that would not advance the offset"""
    sc, un, tracks = _case_tracks(oracle, scenes, "M3-cap70")
    t = tracks["sweep"]
    first, ticks = fref.tracked_ticks(oracle, sc, t, 3)
    same(first, composed(oracle, sc, t), keys=("paths", "n_points", "known", "rot"))
    _, frozen = fref.tracked_ticks(oracle, sc, t, 3, advance=0)
    # the same state in front of the first tick's rollout, another offset
    assert ticks[0][0] == frozen[0][0]
    assert not np.array_equal(ticks[0][1]["paths"], frozen[0][1]["paths"])
    assert all(not np.array_equal(a[1]["paths"], b[1]["paths"]) for a, b in zip(ticks, frozen))


def test_live_list_at_rest_under_moving_tracks(scenes):
    """the case most likely to go wrong on the device: the shapes without `moving` have every field velocity +0.0 in the
    live list (the launcher's test for the bodies that assume obstacles at rest), while their tracks move"""
    for shape, s in fref.SHAPES.items():
        sc = fref.build_scene(scenes, shape)
        at_rest = not np.any(sc["obstacles"][:-1, 3:6])
        assert at_rest == (not s.get("moving")), shape


def test_ftrack_kernels_use_no_scratch(pmaf, hip_lib):
    path = os.path.join(os.path.dirname(os.path.abspath(pmaf.LIB_PATH)), "resource_usage.txt")
    text = open(path).read()
    blocks = re.split(r"(?=Function Name: )", text)
    mine = [b for b in blocks if re.match(r"Function Name: _Z\d+k_rollout_w64_ftrack", b)]
    assert len(mine) == 4, [b.splitlines()[0] for b in mine]
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b
        assert re.search(r"VGPRs Spill: 0\b", b), b
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        assert occ >= 2, b
