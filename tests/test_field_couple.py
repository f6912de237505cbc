"""The obstacle tracks' device-side source (include/pmaf.h "obstacle tracks", pmaf_couple_obstacle_tracks) without a
device: the composition of tests/field_couple_reference.py is held to the contract's identities and to the oracle's own
rollout, every shape group the GPU suite runs (tests/test_field_couple_gpu.py) is shown to be sensitive to each rule of
the contract, and the new kernels' resource record is held to no scratch."""
import os
import re

import numpy as np
import pytest

import field_couple_reference as cref
import field_track_reference as fref
import sentinel_track_reference as sref


@pytest.fixture(autouse=True)
def _portable_exp_oracle(oracle):
    oracle.set_exp_mode(1)
    yield
    oracle.set_exp_mode(0)


def untracked(oracle, sc):
    ora = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
    ora.set_initial_position(sc["start"])
    ora.rollout()
    paths, n = ora.paths()
    return dict(paths=paths, n_points=n, min_obs=ora.min_obs_dist(), known=ora.known(), rot=ora.rot_vecs(), vel=ora.agent_vel(),
                reached=ora.success())


def test_composition_identities(oracle, scenes):
    """scale 1, anchor 0: the attached column's positions are the selected path's bits, held at the end; unattached
    columns are straight_lines for all cap points; the velocity is the forward difference and +0.0 from n_c - 1 on; a
    population whose sources have no selection, or without an attached column, has L = 0"""
    sc = sref.build_scene(scenes, "M3-cap70-moving")
    un = untracked(oracle, sc)
    cap, dt, M = sc["max_prediction_steps"], sc["dt"], 3
    path, n = un["paths"][3], int(un["n_points"][3])
    assert 5 < n <= cap
    lines = fref.straight_lines(sc["obstacles"], dt, cap)
    src, scale, anchor = [1, -1, -1], np.ones(M), np.zeros((M, 3))
    for shift in (0, 1, n - 1, n, n + 4):
        t = cref.compose_tracks([None, path], [0, n], [False, True], src, scale, anchor, shift, sc["obstacles"], dt, cap)
        assert t.shape == (cap, M, 6)
        n_c = max(n - shift, 1)
        first = min(shift, n - 1)
        np.testing.assert_array_equal(t[:n_c, 0, 0:3], path[first:n])
        np.testing.assert_array_equal(t[n_c - 1:, 0, 0:3], np.repeat(path[n - 1:n], cap - n_c + 1, axis=0))
        assert not np.any(t[n_c - 1:, 0, 3:6]) and not np.signbit(t[n_c - 1:, 0, 3:6]).any()
        np.testing.assert_array_equal(t[:n_c - 1, 0, 3:6], (path[first + 1:n] - path[first:n - 1]) / dt)
        np.testing.assert_array_equal(t[:, 1:], lines[:, 1:])
        assert np.any(t[-1, 1, 0:3] != t[0, 1, 0:3])           # the moving unattached column runs to cap
    # anchor and scale: one rounded multiply, one rounded add
    a = np.array([0.1, -0.25, 0.3])
    t = cref.compose_tracks([None, path], [0, n], [False, True], src, [0.7, 1, 1], [a, a, a], 0, sc["obstacles"], dt, cap)
    np.testing.assert_array_equal(t[:n, 0, 0:3], a + np.float64(0.7) * path[:n])
    # no selection yet / nothing attached
    assert cref.compose_tracks([None, path], [0, n], [False, False], src, scale, anchor, 0, sc["obstacles"], dt, cap).shape == (0, M, 6)
    assert cref.compose_tracks([None, path], [0, n], [False, True], [-1] * M, scale, anchor, 0, sc["obstacles"], dt, cap).shape == (0, M, 6)
    # two columns, one of whose sources has no selection: that column counts as unattached
    t = cref.compose_tracks([path, path], [n, n], [False, True], [0, -1, 1], scale, anchor, 0, sc["obstacles"], dt, cap)
    np.testing.assert_array_equal(t[:, 0], lines[:, 0])
    np.testing.assert_array_equal(t[:n, 2, 0:3], path[:n])


def test_reciprocal_multiply_is_not_the_division(oracle, scenes):
    """d * (1 / dt) in place of d / dt: about 13 % of full-mantissa numerators differ at dt = 0.01. The differences of
    two neighbouring path points have lost their low bits to the cancellation, so fewer of THEM differ (0.5 ... 3 % per
    agent here) -- still some on every agent's path, which is what makes the mutant visible in the tick sequences"""
    sc = sref.build_scene(scenes, "M3-cap70")
    assert sc["dt"] == 0.01
    dt = np.float64(sc["dt"])
    d = np.random.default_rng(7).uniform(-0.02, 0.02, 200000)
    generic = float((d / dt != d * (np.float64(1.0) / dt)).mean())
    print("full-mantissa numerators that differ: %.4f" % generic)
    assert 0.10 < generic < 0.16, generic
    un = untracked(oracle, sc)
    M, cap = 3, sc["max_prediction_steps"]
    frac = []
    for i in range(sref.N_AGENTS):
        path, n = un["paths"][i], int(un["n_points"][i])
        args = ([None, path], [0, n], [False, True], [1, -1, -1], np.ones(M), np.zeros((M, 3)), 0, sc["obstacles"], sc["dt"], cap)
        a, b = cref.compose_tracks(*args), cref.compose_tracks(*args, mutant="recip")
        frac.append(float((a[:n - 1, 0, 3:6] != b[:n - 1, 0, 3:6]).mean()))
    print("components that differ per agent:", frac)
    assert min(frac) > 0.0, frac
    # the device suite's getter cases (fast_scenes): the composed tracks tell the two apart, the paths do not
    for shape, shift in (("M3-cap70", 1), ("M59-cap70-moving", 2), ("M60-cap70-lds-general-moving", 1)):
        scs = cref.fast_scenes(scenes, shape)
        att = cref.dual_attach(len(scs[0]["obstacles"]) - 1)
        _, a = cref.field_coupled_ticks(oracle, scs, att[0], att[1], att[2], shift, 2)
        _, b = cref.field_coupled_ticks(oracle, scs, att[0], att[1], att[2], shift, 2, mutant="recip")
        assert all(any(not np.array_equal(x, y) for x, y in zip(ta[1], tb[1])) for ta, tb in zip(a, b)), (shape, shift)


@pytest.mark.parametrize("shape", ["M3-cap70-moving", "M59-cap9-general-moving", "M60-cap70"])
def test_composed_straight_lines_give_the_oracles_rollout(oracle, scenes, shape):
    """the unattached columns of a composition are straight_lines for all cap points, and tracks that are straight
    lines in every column give orc_rollout bit for bit (the one attached column is put back on its line: no scale and
    anchor reproduce a line from a path)"""
    sc = sref.build_scene(scenes, shape)
    want = untracked(oracle, sc)
    M, cap = len(sc["obstacles"]) - 1, sc["max_prediction_steps"]
    far = np.tile(np.array([[50.0, 50.0, 50.0]]), (cap, 1))
    t = cref.compose_tracks([None, far], [0, cap], [False, True], [1] + [-1] * (M - 1), np.ones(M), np.zeros((M, 3)), 0,
                            sc["obstacles"], sc["dt"], cap)
    lines = fref.straight_lines(sc["obstacles"], sc["dt"], cap)
    np.testing.assert_array_equal(t[:, 1:], lines[:, 1:])
    t[:, 0] = lines[:, 0]
    ora = oracle.OraclePlanner(sc, mgr_init_pos=sc["start"])
    ora.set_initial_position(sc["start"])
    got = fref.compose(ora, oracle.eval_order(), sc, sc["obstacles"], t)
    for k in ("paths", "n_points", "min_obs", "known", "rot", "vel", "reached"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# (shape, short, shift) per shape group: tick sequences tests/test_field_couple_gpu.py runs on the device. The shapes of
# the general group that move have a capacity of 9 -- eight steps from rest, in which no rule but the coupling itself
# shows -- so its cases take the 70-point general shape with the moving column added (dual_scenes(moving=True)).
GROUP_CASES = cref.GROUP_CASES
N_TICKS = 3
# d * (1 / dt) against the division: RN(1 / 0.01) is exactly 100, and the difference of two neighbouring path points has
# lost its low bits to the cancellation -- at the 1e-4 m per step of these crossing arms it keeps about 41, so d * 100 is
# exact and equals RN(d / dt) in every component: the mutant is invisible in these tick sequences, tracks included. It
# shows on faster paths (2e-3 m per step: 0.5 ... 3 % of the components), which
# test_reciprocal_multiply_is_not_the_division holds here and the device suite's getter case compares bit for bit.
PATH_MUTANTS = tuple(m for m in cref.MUTANTS if m != "recip")


def _ticks(oracle, scenes, shape, short, shift, mutant=None):
    scs = cref.dual_scenes(scenes, shape, short, moving=True)
    src, scale, anchor = cref.dual_attach(len(scs[0]["obstacles"]) - 1)
    return cref.field_coupled_ticks(oracle, scs, src, scale, anchor, shift, N_TICKS, mutant=mutant)


def _differs(a, b):
    for (_, _, ra), (_, _, rb) in zip(a, b):
        for x, y in zip(ra, rb):
            if not (np.array_equal(x["paths"], y["paths"]) and np.array_equal(x["n_points"], y["n_points"])):
                return True
    return False


@pytest.mark.parametrize("group", list(GROUP_CASES))
def test_cases_are_sensitive(oracle, scenes, group):
    """every mutant of the contract (but the reciprocal: above) changes path bits in at least one case of every shape
    group, every case sees at least one of them, and every case differs from the uncoupled ticks"""
    for shape, _, _ in GROUP_CASES[group]:
        assert shape in sref.SHAPE_GROUPS[group]
    hit = {m: 0 for m in PATH_MUTANTS}
    for shape, short, shift in GROUP_CASES[group]:
        first, want = _ticks(oracle, scenes, shape, short, shift)
        scs = cref.dual_scenes(scenes, shape, short, moving=True)
        _, plain = cref.field_coupled_ticks(oracle, scs, None, None, None, 0, N_TICKS)
        assert _differs(want, plain), (shape, short)
        # the first rollout, before any selection, is the untracked one
        for p in range(2):
            np.testing.assert_array_equal(first[p]["paths"], untracked(oracle, scs[p])["paths"])
        seen = 0
        for m in PATH_MUTANTS:
            _, got = _ticks(oracle, scenes, shape, short, shift, mutant=m)
            if _differs(got, want):
                hit[m] += 1
                seen += 1
        assert seen >= 1, (shape, short)
    print(group, hit)
    assert all(v >= 1 for v in hit.values()), hit


def test_short_source_is_held_while_unattached_columns_move(oracle, scenes):
    """the `short` variant: arm 1's selected path ends after a few points, arm 0's rollout runs on past it"""
    shape = "M3-cap70-moving"
    _, ticks = _ticks(oracle, scenes, shape, 0.13, 1)
    _, _, res = ticks[0]
    # (the tracks of tick 1 come from tick 0's rollouts: the path of the agent tick 1 selects)
    best1, tracks1, res1 = ticks[1]
    n_src = int(res[1]["n_points"][best1[1]])
    t1 = tracks1[0]
    cap = len(t1)
    assert cap == 70 and 2 <= n_src < 45
    n_c = max(n_src - 1, 1)
    assert np.all(t1[n_c - 1:, 0, 0:3] == t1[n_c - 1, 0, 0:3]) and not np.any(t1[n_c - 1:, 0, 3:6])
    assert np.any(t1[cap - 1, 1, 0:3] != t1[n_c - 1, 1, 0:3])
    assert int(res1[0]["n_points"].max()) > n_c + 1            # arm 0 reads the held points


def test_attached_sphere_enters_the_shell_mid_rollout(oracle, scenes):
    """column 0 rides 0.25 m beside the other arm's path: outside every agent's shell at the start of the rollout that
    follows it, inside it later -- the latch happens on a composed position"""
    shape = "M3-cap70"
    scs = cref.dual_scenes(scenes, shape)
    _, ticks = _ticks(oracle, scenes, shape, False, 1)
    r0 = scs[0]["obstacles"][0, 6]
    entered = 0
    for best, tracks, res in ticks:
        for p in range(2):
            for i in range(cref.N_AGENTS):
                n = int(res[p]["n_points"][i])
                d = [fref.shell_distance(scs[p], res[p]["paths"][i, k], tracks[p][k, 0, 0:3], r0) for k in range(n - 1)]
                if d[0] > scs[p]["detect_shell_rad"] and min(d) < scs[p]["detect_shell_rad"]:
                    entered += 1
    assert entered >= 1


def test_fcouple_kernels_use_no_scratch(pmaf, hip_lib):
    path = os.path.join(os.path.dirname(os.path.abspath(pmaf.LIB_PATH)), "resource_usage.txt")
    text = open(path).read()
    blocks = re.split(r"(?=Function Name: )", text)
    mine = [b for b in blocks if re.match(r"Function Name: _Z\d+k_fcouple_(take|compose)", b)]
    assert len(mine) == 2, [b.splitlines()[0] for b in mine]
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b
        assert re.search(r"VGPRs Spill: 0\b", b), b
        assert re.search(r"LDS Size \[bytes/block\]: 0\b", b), b
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        assert occ >= 2, b
    # the names collide with none of the substrings the other modules look their kernels up by
    for other in ("k_select_audit", "k_track_from_best", "k_rollout_w64_ftrack", "k_audit_track"):
        assert not any(other in b.splitlines()[0] for b in mine)
