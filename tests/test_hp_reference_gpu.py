"""Every rollout kernel family and arithmetic policy against the independent high-precision reference
(tests/hp_reference.py), one tick or one stepping call at a time on the HIP path's own fp64 state (tests/hp_shadow.py).

The parity suite holds the strict kernels to the CPU oracle bit for bit and the contracted ones to 1e-5 m end to end;
here each output is held to the reference's rounding-error bound for the policy's documented per-operation error, and
each decided branch to the reference's side. launch_config() confirms which kernel ran. Large shapes compare a seeded
sample of agents (the agents of a rollout are independent). Run with -s to see the per-case report.
"""
import json
import os

import numpy as np
import pytest
import torch

import hp_anchored as ha
import hp_edges
import hp_reference as hp
import hp_shadow as sh

pytestmark = pytest.mark.gpu

POLICY_KW = {"xact": {}, "ieee": {"ieee_sequences": True}, "fast": {"fast_math": True}, "fma": {"contracted": True}}
ONE_STEP_MAX_UNDECIDABLE = 0.02
K_STEP_MAX_UNDECIDABLE = 0.10       # see tests/test_hp_reference.py: the bound of a step near a sphere grows fast


def _simds():
    return torch.cuda.get_device_properties(0).multi_processor_count * 4


def _planner(pmaf, scene, policy, lpa=0):
    return pmaf.PmafPlanner(scene, device=0, mgr_init_pos=scene["start"], lanes_per_agent=lpa, **POLICY_KW[policy])


def _sample(n, k, seed=7):
    if n <= k:
        return list(range(n))
    return sorted(np.random.default_rng(seed).choice(n, k, replace=False).tolist())


def run_ticks(pmaf, scenes, scene, n_ticks, policy, name, lpa=0, dynamic=False, n_sample=16, expect=None):
    A = hp.Arith(policy)
    st = sh.Stats("%s [%s]" % (name, policy))
    pl = _planner(pmaf, scene, policy, lpa)
    try:
        ip = sh.start(pl, scene, init_pos=scene["start"] + np.array([0.0, 0.0, -0.25]), real_pos=scene["start"])
        cfg = pl.launch_config()
        for k, v in (expect or {}).items():
            assert cfg[k] == v, (k, cfg)
        agents = _sample(int(scene["n_agents"]), n_sample)
        obs = scene["obstacles"].copy()
        for _ in range(n_ticks):
            sh.shadow_tick(pl, scene, obs, ip, A, st, agents=agents)
            if dynamic:
                obs = scenes.advance_live_obstacles(obs)
    finally:
        pl.close()
    return st


# ---------------------------------------------------------------------------------------------------------------------
# k_rollout_w64, one obstacle slot per lane (M <= 60)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["xact", "ieee", "fast", "fma"])
def test_w64_one_slot(pmaf, scenes, policy):
    st = run_ticks(pmaf, scenes, scenes.static1_scene(16, 1), 20, policy, "w64 one-slot C1",
                   expect=dict(lanes_per_agent=64, waves_per_agent=1, priority_slices=False))
    st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


@pytest.mark.parametrize("policy", ["xact", "fast", "fma"])
def test_w64_one_slot_dynamic(pmaf, scenes, policy):
    st = run_ticks(pmaf, scenes, scenes.dyn1_scene(10, 1), 20, policy, "w64 one-slot dyn1", dynamic=True,
                   expect=dict(lanes_per_agent=64, waves_per_agent=1))
    st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


def test_w64_one_slot_lds_sum(pmaf, scenes, monkeypatch):
    monkeypatch.setenv("PMAF_SUM", "lds")
    st = run_ticks(pmaf, scenes, scenes.dyn1_scene(10, 1), 20, "xact", "w64 one-slot LDS sum", dynamic=True,
                   expect=dict(lanes_per_agent=64, waves_per_agent=1))
    st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


@pytest.mark.parametrize("policy", ["xact", "fma"])
def test_w64_k_step(pmaf, scenes, policy):
    st = run_ticks(pmaf, scenes, scenes.static1_scene(16, 20), 2, policy, "w64 C1 20-step",
                   expect=dict(lanes_per_agent=64, waves_per_agent=1))
    st.assert_ok(K_STEP_MAX_UNDECIDABLE)


@pytest.mark.parametrize("policy", ["xact", "fast"])
def test_w64_general_step(pmaf, scenes, monkeypatch, policy):
    """PMAF_PLAIN_STEP=0: the general step, with a non-unit mass and agents without attraction"""
    monkeypatch.setenv("PMAF_PLAIN_STEP", "0")
    sc = scenes.dyn1_scene(10, 6)
    sc["agent_mass"] = 1.5
    sc["k_attr"] = np.array([4.0, 0.0, 4.0, 4.0, 0.0, 4.0, 3.0, 0.0, 4.0, 5.0])
    st = run_ticks(pmaf, scenes, sc, 6, policy, "w64 general step", dynamic=True,
                   expect=dict(lanes_per_agent=64, waves_per_agent=1))
    st.assert_ok(K_STEP_MAX_UNDECIDABLE)


@pytest.mark.parametrize("policy,m", [("xact", 62), ("fma", 64), ("xact", 200), ("fma", 128)])
def test_w64_tiles(pmaf, scenes, monkeypatch, policy, m):
    """2-4 obstacle tiles per lane of the one-wave kernel (PMAF_MW=0 keeps it for M = 61..256)"""
    monkeypatch.setenv("PMAF_MW", "0")
    sc = scenes.synthetic_scene(16, 1, m, 7, m, dynamic=True)
    st = run_ticks(pmaf, scenes, sc, 4, policy, "w64 tiles M=%d" % m, dynamic=True, n_sample=8,
                   expect=dict(lanes_per_agent=64, waves_per_agent=1))
    st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


def test_w64_sliced(pmaf, scenes):
    """k_rollout_w64_sliced: one-slot rollouts between one and two waves per SIMD of this device"""
    simds = _simds()
    for policy in ("xact", "fma"):
        sc = scenes.synthetic_scene(simds + simds // 2, 1, 24, 8, 1, dynamic=True)
        st = run_ticks(pmaf, scenes, sc, 3, policy, "w64 sliced", dynamic=True, lpa=64, n_sample=16,
                       expect=dict(lanes_per_agent=64, waves_per_agent=1, priority_slices=True))
        st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


# ---------------------------------------------------------------------------------------------------------------------
# k_rollout_mw, k_rollout_grp, generic k_rollout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [2, 3, 4])
@pytest.mark.parametrize("policy", ["xact", "fast", "fma"])
def test_mw(pmaf, scenes, monkeypatch, waves, policy):
    monkeypatch.setenv("PMAF_MW", str(waves))
    sc = scenes.synthetic_scene(14, 1, 100, 7, 100, dynamic=True)
    st = run_ticks(pmaf, scenes, sc, 3, policy, "mw W=%d" % waves, dynamic=True, n_sample=6,
                   expect=dict(waves_per_agent=waves))
    st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


@pytest.mark.parametrize("lpa", [8, 16, 32])
@pytest.mark.parametrize("policy", ["xact", "fma"])
def test_grp(pmaf, scenes, lpa, policy):
    sc = scenes.synthetic_scene(64, 1, 32, 2, 0, dynamic=True)
    st = run_ticks(pmaf, scenes, sc, 4, policy, "grp LPA %d" % lpa, lpa=lpa, dynamic=True, n_sample=12,
                   expect=dict(lanes_per_agent=lpa))
    st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


def test_grp_k_step(pmaf, scenes):
    sc = scenes.synthetic_scene(64, 12, 32, 2, 0, dynamic=True)
    st = run_ticks(pmaf, scenes, sc, 2, "xact", "grp LPA 16 12-step", lpa=16, dynamic=True, n_sample=8,
                   expect=dict(lanes_per_agent=16))
    st.assert_ok(K_STEP_MAX_UNDECIDABLE)


@pytest.mark.parametrize("lpa", [64, 16, 8])
def test_generic(pmaf, scenes, monkeypatch, lpa):
    monkeypatch.setenv("PMAF_FORCE_GENERIC", "1")
    st = run_ticks(pmaf, scenes, scenes.dyn1_scene(10, 1), 10, "xact", "generic LPA %d" % lpa, lpa=lpa, dynamic=True,
                   expect=dict(lanes_per_agent=lpa))
    st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


# ---------------------------------------------------------------------------------------------------------------------
# k_plan_steps, k_link_force, k_eval_obstacle_distance, exact ties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpa", [0, 16, 1])
def test_stepping_api(pmaf, scenes, lpa):
    A = hp.Arith("xact")
    st = sh.Stats("stepping API LPA %d" % lpa)
    sc = scenes.synthetic_scene(8, 40, 16, config_id=2, dynamic=True)
    pl = _planner(pmaf, sc, "xact", lpa)
    try:
        ip = sh.start(pl, sc)
        pl.set_agent_pos_and_vels(np.array([-0.2, 0.05, 0.68]), np.array([0.15, -0.01, 0.02]))
        sh.shadow_steps(pl, sc, sc["obstacles"], ip, A, st, 15)
    finally:
        pl.close()
    st.assert_ok(ONE_STEP_MAX_UNDECIDABLE)


def test_link_force_and_eval_obstacle_distance(pmaf, scenes):
    A = hp.Arith("xact")
    st = sh.Stats("link_force / eval_obstacle_distance")
    sc = scenes.static1_scene(16, 4)
    obs = sc["obstacles"].copy()
    obs[-1, :3] = [0.1, 0.05, 0.8]
    rng = np.random.default_rng(5)
    lp = obs[-1, :3] + rng.uniform(-0.4, 0.4, (48, 3))
    lp[0] = obs[-1, :3]
    lp[1] = obs[-1, :3] + [0.0, 0.0, 0.5]
    lp[2] = obs[-1, :3] + [0.0, 0.0, 0.15]
    kr = rng.uniform(0.01, 0.1, 48)
    pl = _planner(pmaf, sc, "xact")
    try:
        sh.start(pl, sc)
        sh.shadow_link_force(pl, sc, lp, kr, obs, A, st)
        for p in lp[::6]:
            pl.set_agent_positions(p)
            sh.shadow_eval_obstacle_distance(pl, sc, obs, A, st)
    finally:
        pl.close()
    st.assert_ok(0.02)


@pytest.mark.parametrize("kernel", ["default", "grp16", "generic"])
def test_exact_tie_scenes(pmaf, monkeypatch, kernel):
    """each tie decided with bound 0 by the reference; the kernel takes the same side"""
    lpa = 16 if kernel == "grp16" else 0
    if kernel == "generic":
        monkeypatch.setenv("PMAF_FORCE_GENERIC", "1")
        lpa = 64
    A = hp.Arith("xact")
    st = sh.Stats("exact-tie scenes, %s" % kernel)
    for edge in hp_edges.EDGES:
        edge.run(lambda sc: _planner(pmaf, sc, "xact", lpa), A, st)
    st.assert_ok(0.0)


# ---------------------------------------------------------------------------------------------------------------------
# anchored walks: every step of full-length rollouts, every population (tests/hp_anchored.py)
# ---------------------------------------------------------------------------------------------------------------------
ANCHORED_MAX_UNDECIDABLE = 0.02


def _anchored(pmaf, scenes, scs, n_ticks, policy, name, agents, frac, lpa=0, expect=None, dynamic=False, walk_from=0,
              host_coupling=False, mailbox=False, eval_agents=None):
    """n_ticks ticks of one handle holding the populations `scs`; from tick walk_from on, the sampled agents of every
    population are walked. host_coupling: C4 coupled on the host (shard.DualArmCoupling rows); mailbox: coupled inside the
    handle through its peer mailbox, the shadow rebuilding the trailing rows. eval_agents="all": every agent's cost and
    the selected index are compared (hp_shadow.shadow_tick) in the first tick (one-point paths: the whole population
    ties and index 0 must win) and in the last one (full-length paths)"""
    A = hp.Arith(policy)
    st = sh.Stats("%s [%s]" % (name, policy))
    st.evaluation = sh.Stats("%s [%s], every cost and the selection" % (name, policy))   # (its own counts: st's cap is unchanged)
    single = len(scs) == 1
    starts = np.stack([s["start"] for s in scs])
    pl = pmaf.PmafPlanner(scs[0] if single else scs, device=0, mgr_init_pos=starts[0] if single else starts,
                          lanes_per_agent=lpa, **POLICY_KW[policy])
    try:
        if single:
            ip = sh.start(pl, scs[0], init_pos=starts[0] + np.array([0.0, 0.0, -0.25]), real_pos=starts[0])
        else:
            pl.set_initial_position(starts)
            ip = starts
        cfg = pl.launch_config()
        for k, v in (expect or {}).items():
            assert (cfg[k] >= 2) if v == ">=2" else (cfg[k] == v), (k, cfg)
        coupling = None
        if mailbox:
            pmaf.shard.connect_peers(pl, None, 1, 0)
            pmaf.shard.couple_dual_arm_on_device(pl, 1, 0, starts)
            coupling = {0: (1, 0.1), 1: (0, 0.1)}
        obs = np.stack([s["obstacles"] for s in scs])
        host = pmaf.shard.DualArmCoupling(obs, 0.1) if host_coupling else None
        for t in range(n_ticks):
            rows = host.coupled_obstacles(pl.real_state()[0]) if host else obs
            ag = agents(pl) if callable(agents) else agents
            sh.shadow_tick(pl, scs[0] if single else scs, rows[0] if single else rows, ip, A, st,
                           agents=ag if t >= walk_from else [], rollouts=ha.walker(frac, seed=t), coupling=coupling,
                           eval_agents=eval_agents if t in (0, n_ticks - 1) else None, eval_stats=st.evaluation)
            if dynamic:
                obs = np.stack([scenes.advance_live_obstacles(o) for o in obs])
        if mailbox:
            pl.stop()
            pl.peer_disconnect()
    finally:
        pl.close()
    return st


def _assert_anchored(st, min_horizon):
    assert st.walk.horizon >= min_horizon, st.report()
    st.assert_ok(ANCHORED_MAX_UNDECIDABLE, min_compared=4)


@pytest.mark.parametrize("policy", ["xact", "fma", "fast"])
def test_anchored_c2_w64_one_slot(pmaf, scenes, policy):
    """BASELINE C2 (the bench headline: 64 agents, H = 200, 32 spheres) on k_rollout_w64, one obstacle slot per lane.
    Every agent's cost and the selected index are compared in the first and the last tick. Measured with the oracle in
    the planner's place on one CPU core: 64 paths of 200 points cost 5.1 s per tick (99.0 s with all three ticks widened
    against 88.8 s with the 8 walked agents' costs only), so one full-length tick is widened: + 5 s. C4 (10.7 s per arm
    and tick for its 256 paths) and C5 stay sampled."""
    st = _anchored(pmaf, scenes, [scenes.config_scene("C2")], 3, policy, "anchored C2 w64 one-slot",
                   _sample(64, 8), 0.15, expect=dict(lanes_per_agent=64, waves_per_agent=1, priority_slices=False),
                   eval_agents="all")
    _assert_anchored(st, 200)
    st.evaluation.assert_ok(0.0, min_compared=2 * 65)
    assert st.evaluation.selections == 2, st.evaluation.report()


@pytest.mark.parametrize("policy", ["xact", "fma"])
def test_anchored_c3_mw(pmaf, scenes, policy):
    """BASELINE C3 (256 agents, H = 500, 128 spheres) on k_rollout_mw at its default wave count"""
    st = _anchored(pmaf, scenes, [scenes.config_scene("C3")], 1, policy, "anchored C3 mw", _sample(256, 4), 0.04,
                   expect=dict(waves_per_agent=">=2"))
    _assert_anchored(st, 400)


@pytest.mark.parametrize("policy", ["xact", "fma"])
def test_anchored_c5_grp(pmaf, scenes, policy):
    """BASELINE C5 at full size: 8 populations x 1024 agents on k_rollout_grp, 16 lanes per agent; 2 agents of every
    population (scene 1, the chaotic one, included)"""
    scs = [scenes.config_scene("C5", scene_id=s) for s in range(8)]
    st = _anchored(pmaf, scenes, scs, 2, policy, "anchored C5 8x1024 grp LPA 16", _sample(1024, 2, seed=11), 0.15,
                   lpa=16, expect=dict(lanes_per_agent=16), walk_from=1)
    _assert_anchored(st, 150)


def test_anchored_c5x2_sliced(pmaf, scenes):
    """two C5 scenes in one handle: k_rollout_w64_sliced (priority slices)"""
    scs = [scenes.config_scene("C5", scene_id=s) for s in (0, 2)]
    st = _anchored(pmaf, scenes, scs, 2, "fma", "anchored C5x2 w64 sliced", _sample(1024, 2, seed=12), 0.15,
                   expect=dict(lanes_per_agent=64, priority_slices=True))
    _assert_anchored(st, 150)


def test_anchored_c4_host_coupling(pmaf, scenes):
    """BASELINE C4: two arms, each arm's trailing obstacle the other arm's end effector, coupled on the host"""
    st = _anchored(pmaf, scenes, scenes.dual_arm_scenes(), 3, "xact", "anchored C4 host coupling",
                   _sample(256, 2, seed=13), 0.15, host_coupling=True)
    _assert_anchored(st, 150)


def test_anchored_c4_peer_mailbox(pmaf, scenes):
    """BASELINE C4 coupled inside one handle through its peer mailbox: the shadow rebuilds each population's trailing
    row from the other population's previous real position"""
    st = _anchored(pmaf, scenes, scenes.dual_arm_scenes(), 3, "fma", "anchored C4 peer mailbox",
                   _sample(256, 2, seed=13), 0.15, mailbox=True)
    _assert_anchored(st, 150)


@pytest.mark.parametrize("task", ["sim_kobo_dyn_spheres1", "sim_kobo_dyn_spheres2", "sim_kobo_dyn_spheres3"])
def test_anchored_shipped_tasks(pmaf, scenes, task):
    """the reference's shipped sim_kobo scenes (10 agents, H = 1500 / 1200, moving spheres): the agent selected last
    tick and one more, sampled steps"""
    recs = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "task_scenes.json")))
    sc = scenes.scene_from_record(recs[task], task)

    def best_plus_one(pl):
        b = max(pl.best_id() - 1, 0)
        return [b, (b + 5) % 10]
    st = _anchored(pmaf, scenes, [sc], 2, "fma", "anchored %s" % task, best_plus_one, 0.08, dynamic=True,
                   walk_from=1)
    _assert_anchored(st, 500)            # a rollout that reaches the goal ends there (sim_kobo_dyn_spheres2: 915 steps)
