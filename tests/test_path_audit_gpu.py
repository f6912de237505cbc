"""Path audit on the GPU (pmaf_evaluate_paths / pmaf_evaluate_path, include/pmaf.h) through the C-ABI against
tests/path_audit_reference.py at TOLERANCE 0: integers equal, doubles bit-equal, a NaN matched by a NaN; no case is
skipped. The reference takes its dot association from pmaf_eval_order(), so the file passes unchanged under
PMAF_VARIANT=rassoc."""
import ctypes as C

import numpy as np
import pytest

import path_audit_reference as ref

pytestmark = pytest.mark.gpu

KEYS = ("clearance", "step", "obstacle", "first_violation", "per_obstacle")


def _same_bits(got, want, what):
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float64).reshape(got.shape))
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), "%s: %d of %d values differ, first at %s: %r != %r" % (
        what, (~ok).sum(), ok.size, np.argwhere(~ok)[0], got[~ok][0], want[~ok][0])


def _shaped(pl, a, tail=()):
    return np.asarray(a).reshape((pl.P, pl.N) + tuple(tail))


def check_against_reference(pl, sc, obs, margin, hip_lib):
    """one audit call compared with the reference on the handle's own paths; returns (got, want)"""
    obs = np.asarray(obs, dtype=np.float64).reshape(pl.P, pl.n_obs, 7)
    got = pl.evaluate_paths(obs, margin, per_obstacle=True)
    paths, n = pl.paths()
    paths, n = _shaped(pl, paths, (pl.cap, 3)), _shaped(pl, n)
    want = ref.audit(paths.tolist(), n.tolist(), obs.tolist(), sc["dt"], sc.get("radius", 0.05), margin,
                     hip_lib.pmaf_eval_order())
    for k in ("step", "obstacle", "first_violation"):
        np.testing.assert_array_equal(_shaped(pl, got[k]), np.asarray(want[k]), err_msg=k)
    _same_bits(_shaped(pl, got["clearance"]), want["clearance"], "clearance")
    _same_bits(_shaped(pl, got["per_obstacle"], (pl.n_obs,)), want["per_obstacle"], "per_obstacle")
    # the optional outputs left out: the same clearance
    lean = pl.evaluate_paths(obs, margin)
    assert "per_obstacle" not in lean
    _same_bits(lean["clearance"], got["clearance"], "clearance without per_obstacle")
    _same_bits(np.asarray(got["per_obstacle"]).min(axis=-1), got["clearance"], "per_obstacle.min == clearance")
    return {k: _shaped(pl, got[k], (pl.n_obs,) if k == "per_obstacle" else ()) for k in KEYS}, n


def rollout_case(pmaf, scenes, P, N, M, H, ragged=False):
    """P differing synthetic scenes, every obstacle moving (the trailing one too); returns planner, scenes, start list"""
    scs = []
    for p in range(P):
        sc = scenes.synthetic_scene(N, H, M, config_id=7, scene_id=p, dynamic=True)
        sc["obstacles"][-1] = [0.05 * p, 0.2, 0.8, -0.04, 0.03 + 0.01 * p, -0.02, 0.1]
        if ragged:   # close to the goal, agents of different stiffness: some rollouts end at the goal guard, some do not
            sc["start"] = sc["goal"] - np.array([0.13, 0.01 * p, 0.0])
            sc["k_attr"] = np.linspace(1.0, 8.0, N)
        scs.append(sc)
    starts = np.stack([s["start"] for s in scs])
    pl = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    pl.set_initial_position(starts)
    pl.rollout()
    return pl, scs, np.stack([s["obstacles"] for s in scs])


def live_list(scenes, start):
    """the tick's fresh list: the start list one node period later, the trailing obstacle moved as well"""
    live = np.stack([scenes.advance_live_obstacles(o) for o in start])
    live[:, -1, 0:3] += np.array([0.01, -0.02, 0.005])
    return live


# field obstacles 2 / 66: within / past one wave of lanes; horizon 8 / 70: fewer / more path points than one pass of a
# block covers (4 waves x 64 / G points); N = 5; P = 2 with differing scenes
@pytest.mark.parametrize("P,N,M,H,ragged", [(2, 5, 2, 8, False), (2, 5, 66, 70, False), (1, 5, 66, 8, False),
                                            (2, 5, 2, 70, True), (1, 5, 31, 70, False), (1, 1, 0, 8, False)])
def test_rollout_paths_against_the_advanced_list(pmaf, scenes, hip_lib, P, N, M, H, ragged):
    pl, scs, start = rollout_case(pmaf, scenes, P, N, M, H, ragged)
    try:
        got, n = check_against_reference(pl, scs[0], live_list(scenes, start), 0.06, hip_lib)
        print("n_points", n.tolist(), "clearance", got["clearance"].tolist(), "step", got["step"].tolist(),
              "obstacle", got["obstacle"].tolist(), "first_violation", got["first_violation"].tolist())
        if ragged:
            assert len(set(n.reshape(-1).tolist())) > 1, "the case is meant to have paths of different lengths: %s" % n
            assert n.min() < H + 1
        else:
            assert (n == H + 1).all()
        assert (got["step"] < n).all() and (got["step"] >= 0).all()
    finally:
        pl.close()


def rest_planner(pmaf, scenes, obstacles, pos, N=1, steps=6, dt=0.125, radius=0.125):
    """agents with all gains 0, set at rest at `pos`, stepped `steps` times through static far obstacles: steps + 1
    identical path points"""
    obstacles = np.asarray(obstacles, dtype=np.float64)
    sc = scenes.synthetic_scene(N, 8, obstacles.shape[0] - 1)
    sc.update(obstacles=obstacles, dt=dt, radius=radius, k_attr=0.0, k_circ=0.0, k_repel=0.0, k_damp=0.0,
              start=np.asarray(pos, dtype=np.float64), goal=np.asarray(pos, dtype=np.float64) + np.array([0.5, 0.0, 0.0]))
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    pl.set_agent_pos_and_vels(sc["start"], np.zeros(3))
    still = obstacles.copy()
    still[:, 3:6] = 0.0
    pl.move_agents(still, dt, steps)
    paths, n = pl.paths()
    paths, n = _shaped(pl, paths, (pl.cap, 3)), _shaped(pl, n)
    assert (n == steps + 1).all()
    assert (paths[:, :, :steps + 1] == sc["start"]).all(), "the agents were meant to stay at rest"
    return pl, sc


def test_hand_derived_moving_obstacle(pmaf, scenes, hip_lib):
    """an agent at rest at the origin, ONE obstacle (P = N = n_obstacles = 1) at (1, 0, 0) with v = (-0.5, 0, 0),
    dt 0.125, radii 0.125 + 0.25: c(k) = (1 - 0.0625 k) - 0.375 exactly (tests/test_path_audit.py derives it)"""
    moving = [[1.0, 0.0, 0.0, -0.5, 0.0, 0.0, 0.25]]
    pl, sc = rest_planner(pmaf, scenes, moving, [0.0, 0.0, 0.0])
    try:
        r = pl.evaluate_paths(moving, 0.45, per_obstacle=True)
        assert float(r["clearance"][0]) == 0.25 and int(r["step"][0]) == 6 and int(r["obstacle"][0]) == 0
        assert int(r["first_violation"][0]) == 3 and r["per_obstacle"].tolist() == [[0.25]]
        for margin, fv in ((0.4375, 4), (0.25, 7), (1.0, 0), (0.0, 7), (-1.0, 7)):
            assert int(pl.evaluate_paths(moving, margin)["first_violation"][0]) == fv, margin
        check_against_reference(pl, sc, moving, 0.45, hip_lib)
    finally:
        pl.close()


def test_tie_over_obstacles_goes_to_the_smaller_index(pmaf, scenes, hip_lib):
    twin = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.25]
    obs = [[0.0, 9.0, 0.0, 0.0, 0.0, 0.0, 0.25], twin, twin, [9.0, 9.0, 9.0, 0.0, 0.0, 0.0, 0.1]]
    pl, sc = rest_planner(pmaf, scenes, obs, [0.0, 0.0, 0.0], N=3)
    try:
        got, _ = check_against_reference(pl, sc, obs, 0.0, hip_lib)
        assert (got["obstacle"] == 1).all() and (got["step"] == 0).all() and (got["clearance"] == 0.625).all()
        assert (got["per_obstacle"][..., 1] == got["per_obstacle"][..., 2]).all()
    finally:
        pl.close()


def test_tie_over_steps_goes_to_the_first_step(pmaf, scenes, hip_lib):
    obs = [[0.3, 2.0, 0.1, 0.0, 0.0, 0.0, 0.25], [5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 0.1]]
    pl, sc = rest_planner(pmaf, scenes, obs, [0.25, -0.5, 0.125], N=2)
    try:
        got, _ = check_against_reference(pl, sc, obs, 0.0, hip_lib)
        c = float(got["clearance"][0, 0])
        assert (got["step"] == 0).all() and (got["obstacle"] == 0).all() and (got["first_violation"] == 7).all()
        above, _ = check_against_reference(pl, sc, obs, c * 1.0000001, hip_lib)
        assert (above["first_violation"] == 0).all()
        at, _ = check_against_reference(pl, sc, obs, c, hip_lib)      # strict `<`: a margin AT the clearance is kept
        assert (at["first_violation"] == 7).all()
    finally:
        pl.close()


def test_margin_sweep_is_monotone(pmaf, scenes, hip_lib):
    pl, scs, start = rollout_case(pmaf, scenes, 1, 5, 9, 40)
    try:
        live = live_list(scenes, start)
        prev = None
        for margin in (-0.5, 0.0, 0.02, 0.05, 0.1, 0.2, 0.4, 0.8, 3.0):
            got, n = check_against_reference(pl, scs[0], live, margin, hip_lib)
            fv = got["first_violation"]
            if prev is not None:
                assert (fv <= prev).all(), (margin, fv, prev)
            prev = fv
        assert (prev == 0).all()                          # every clearance is below 3 m at step 0
        neg = pl.evaluate_paths(live, -0.5)["first_violation"]
        assert (np.asarray(neg) == n.reshape(-1)).all()   # ... and none below -0.5 m
    finally:
        pl.close()


def test_nan_path_points_never_win(pmaf, scenes, hip_lib):
    """Had agents heading straight at an obstacle centred on the start-goal line latch a NaN rotation vector
    (B/src/cf_agent.cpp:599-611): the paths turn NaN from there on. Those pairs never win and never violate."""
    sc = scenes.synthetic_scene(3, 60, 1, 9, 2)
    sc["start"] = np.array([-0.44, 0.0, 0.7])
    sc["goal"] = np.array([0.6, 0.0, 0.7])
    sc["obstacles"][0] = [0.0, 0.0, 0.7, 0, 0, 0, 0.05]
    sc["agent_types"] = np.full(3, 6, dtype=np.int32)
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        pl.rollout()
        paths, n = pl.paths()
        nan_pts = [int(np.isnan(paths[a, :n[a]]).any(axis=-1).sum()) for a in range(3)]
        print("NaN path points per agent", nan_pts, "of", n.tolist())
        assert min(nan_pts) > 0 and all(k < m for k, m in zip(nan_pts, n.tolist()))
        got, _ = check_against_reference(pl, sc, sc["obstacles"], 10.0, hip_lib)
        assert np.isfinite(got["clearance"]).all() and (got["first_violation"] == 0).all()
        assert (got["step"].reshape(-1) < n - np.asarray(nan_pts)).all()
    finally:
        pl.close()


def test_audit_brackets_the_rollouts_min_obs_dist(pmaf, scenes, hip_lib):
    """with the audit list equal to the rollout's start list the audit sees every pair the rollout recorded
    (field obstacles, ungated steps, floored at 1e-5, capped at the shell) and more"""
    for M, H in ((9, 70), (66, 40)):
        pl, scs, start = rollout_case(pmaf, scenes, 2, 5, M, H)
        try:
            got, _ = check_against_reference(pl, scs[0], start, 0.0, hip_lib)
            field = got["per_obstacle"][..., :-1].min(axis=-1)
            bound = np.minimum(scs[0]["detect_shell_rad"], np.maximum(field, 1e-5))
            mo = _shaped(pl, pl.min_obs_dist())
            print("audit bound", bound.tolist(), "min_obs_dist", mo.tolist())
            assert (bound <= mo).all()
        finally:
            pl.close()


def test_evaluate_path_is_the_selected_agents_clearance(pmaf, scenes, hip_lib):
    scs = [scenes.synthetic_scene(6, 30, 5, config_id=7, scene_id=p, dynamic=True) for p in range(2)]
    starts = np.stack([s["start"] for s in scs])
    obs = np.stack([s["obstacles"] for s in scs])
    pl = pmaf.PmafPlanner(scs, device=0, mgr_init_pos=starts)
    try:
        pl.set_initial_position(starts)
        with pytest.raises(pmaf.PmafError) as e:      # no selection yet
            pl.evaluate_path(obs)
        assert e.value.code == -3
        pl.rollout()
        with pytest.raises(pmaf.PmafError) as e:
            pl.evaluate_path(obs)
        assert e.value.code == -3
        best = pl.tick(obs, scs[0]["dt"], scs[0]["cost_gains"], scs[0]["ws_limits"])
        live = live_list(scenes, obs)
        got, _ = check_against_reference(pl, scs[0], live, 0.0, hip_lib)
        sel = np.asarray(pl.evaluate_path(live))
        _same_bits(sel, [got["clearance"][p, best[p]] for p in range(2)], "evaluate_path")
    finally:
        pl.close()


def test_argument_validation(pmaf, scenes, hip_lib):
    sc = scenes.synthetic_scene(4, 10, 3, config_id=7)
    pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
    try:
        pl.set_initial_position(sc["start"])
        pl.rollout()
        L, h = hip_lib, pl._h
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        obs = np.ascontiguousarray(sc["obstacles"], dtype=np.float64)
        clr = np.zeros(4)
        st, ob, fv = (np.zeros(4, dtype=np.int32) for _ in range(3))
        po = np.zeros((4, 4))
        o_p, c_p = obs.ctypes.data_as(dp), clr.ctypes.data_as(dp)
        assert L.pmaf_evaluate_paths(h, None, 0.0, c_p, None, None, None, None) == -1       # NULL list
        assert L.pmaf_evaluate_paths(h, o_p, 0.0, None, None, None, None, None) == -1       # NULL clearance
        assert L.pmaf_evaluate_paths(None, o_p, 0.0, c_p, None, None, None, None) == -1
        assert L.pmaf_evaluate_path(h, None, c_p) == -1 and L.pmaf_evaluate_path(h, o_p, None) == -1
        bad = obs.copy()
        bad[1, 4] = np.nan
        assert L.pmaf_evaluate_paths(h, bad.ctypes.data_as(dp), 0.0, c_p, None, None, None, None) == -1
        assert b"range" in L.pmaf_last_error()
        assert L.pmaf_evaluate_paths(h, o_p, float("nan"), c_p, None, None, None, None) == -1
        # NULL optional outputs are accepted, in every combination tried, and change nothing of the others
        assert L.pmaf_evaluate_paths(h, o_p, 0.05, c_p, st.ctypes.data_as(ip), ob.ctypes.data_as(ip), fv.ctypes.data_as(ip),
                                     po.ctypes.data_as(dp)) == 0
        full = clr.copy()
        for mask in range(8):
            clr[:] = 0.0
            s2, o2, f2 = (np.full(4, -7, dtype=np.int32) for _ in range(3))
            args = [a.ctypes.data_as(ip) if mask >> i & 1 else None for i, a in enumerate((s2, o2, f2))]
            assert L.pmaf_evaluate_paths(h, o_p, 0.05, c_p, args[0], args[1], args[2], None) == 0
            _same_bits(clr, full, "clearance")
            for i, (a, want) in enumerate(((s2, st), (o2, ob), (f2, fv))):
                np.testing.assert_array_equal(a, want if mask >> i & 1 else np.full(4, -7))
    finally:
        pl.close()


def test_an_audit_between_ticks_changes_nothing(pmaf, scenes, hip_lib):
    """best indices and set-points of 5 ticks on C1, with and without audit calls in between: bit-identical"""
    sc = scenes.config_scene("C1")
    runs = []
    for audit in (False, True):
        pl = pmaf.PmafPlanner(sc, device=0, mgr_init_pos=sc["start"])
        try:
            pl.set_initial_position(sc["start"])
            rec = []
            for t in range(5):
                b = pl.tick(sc["obstacles"], sc["dt"], sc["cost_gains"], sc["ws_limits"])
                rec.append((int(b), pl.last_next_pos.copy(), pl.last_next_vel.copy()))
                if audit:
                    live = scenes.advance_live_obstacles(sc["obstacles"])
                    pl.evaluate_paths(live, 0.05, per_obstacle=(t % 2 == 0))
                    pl.evaluate_path(live)
            runs.append(rec)
        finally:
            pl.close()
    for (b0, p0, v0), (b1, p1, v1) in zip(*runs):
        assert b0 == b1
        _same_bits(p1, p0, "set-point position")
        _same_bits(v1, v0, "set-point velocity")
