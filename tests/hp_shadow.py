"""Shadowing a planner with the high-precision reference (tests/hp_reference.py), one tick or one stepping call at a
time, on the planner's OWN fp64 state read back through its getters: every comparison starts from exact inputs, so an
error never compounds across ticks and no chaotic amplification comes into play.

The planner is anything with the CfManager surface of oracle/orc.py:OraclePlanner and the package's PmafPlanner:
one population, or P populations (attribute P > 1; every getter then returns a [P, ...] array, best() the per-population
types and ids). Multi-population calls take the list of P scene dicts, obstacle rows [P, M, 7] and init_pos [P, 3].
Passing rule: |planner - reference| <= BOUND_FACTOR * bound on every compared component, and the planner takes the
reference's side of every branch the reference decides.
"""
import numpy as np

import hp_reference as hp

# the constant factor on the carried bound. The bound is rigorous for a policy whose every operation has relative error
# <= eps (products keep their second-order term, quotients and roots take the worst end of the input interval), so the
# factor is 1: a kernel outside its documented per-operation error fails.
BOUND_FACTOR = 1.0


class Stats:
    """per-case counts: compared / undecidable samples, worst error-to-bound ratio, branch outcomes seen"""

    def __init__(self, name):
        self.name = name
        self.compared = 0
        self.undecidable = 0
        self.undecided_at = {}
        self.worst = 0.0
        self.worst_at = ""
        self.components = 0
        self.seen = {}
        self.failures = []
        self.selections = 0       # compared "best index" samples (check_evaluate)
        self.notes = []           # callables returning extra report lines (tests/hp_anchored.py)

    def merge_seen(self, seen):
        for k, v in seen.items():
            self.seen.setdefault(k, set()).update(v)

    def check(self, label, q, x):
        self.components += 1
        r = hp.excess(q, x)
        if r > self.worst:
            self.worst, self.worst_at = r, label
        if r > BOUND_FACTOR:
            self.failures.append("%s: planner %r, reference %s (error / bound = %.3g)" % (label, float(x), q, r))

    def check_vec(self, label, qv, x):
        for k in range(3):
            self.check("%s[%d]" % (label, k), qv[k], x[k])

    def expect(self, label, want, got):
        self.components += 1
        if want != got:
            self.failures.append("%s: planner %r, reference %r" % (label, got, want))

    def run(self, A, fn):
        """evaluate one sample: fn() raises hp.Undecidable -> counted, nothing compared"""
        A.seen = {}
        fails0, comps0, worst0 = len(self.failures), self.components, (self.worst, self.worst_at)
        try:
            fn()
        except hp.Undecidable as e:
            del self.failures[fails0:]
            self.components = comps0
            self.worst, self.worst_at = worst0
            self.undecidable += 1
            self.undecided_at[str(e)] = self.undecided_at.get(str(e), 0) + 1
            return False
        self.compared += 1
        self.merge_seen(A.seen)
        return True

    def undecidable_fraction(self):
        n = self.compared + self.undecidable
        return self.undecidable / n if n else 0.0

    def report(self):
        lines = ["[%s] compared %d, undecidable %d %s, components %d, worst error/bound %.3g (%s)" % (
            self.name, self.compared, self.undecidable, self.undecided_at or "", self.components, self.worst,
            self.worst_at)]
        lines.append("    branches: " + " ".join("%s:%s" % (b, "".join(sorted("TF"[not o] for o in self.seen.get(b, ()))) or "-")
                                           for b in hp.BRANCHES))
        lines += [f() for f in self.notes]
        return "\n".join(lines)

    def assert_ok(self, max_undecidable=0.05, min_compared=1):
        print(self.report())
        assert not self.failures, "%d mismatches, first: %s" % (len(self.failures), "\n".join(self.failures[:8]))
        assert self.compared >= min_compared, self.report()
        assert self.undecidable_fraction() <= max_undecidable, self.report()


def _gains(scene, i):
    return tuple(float(np.broadcast_to(np.asarray(scene[k], dtype=np.float64), (int(scene["n_agents"]),))[i])
                 for k in ("k_attr", "k_circ", "k_repel", "k_damp"))


def agent_types(scene):
    t = scene.get("agent_types")
    if t is not None:
        return [int(x) for x in t]
    head = [hp.HAD, hp.GOAL, hp.OBSTACLE, hp.GOAL_OBSTACLE, hp.VEL]
    n = int(scene["n_agents"])
    return (head + [hp.RANDOM] * max(0, n - 5))[:n]


def _params(scene):
    return dict(shell=scene["detect_shell_rad"], mass=scene.get("agent_mass", 1.0), rad=scene.get("radius", 0.05),
                vel_max=scene["velocity_max"], approach=scene["approach_dist"])


def start(planner, scene, init_pos=None, real_pos=None):
    """CfManager::setInitialPosition(init_pos) (every agent's and the real agent's init_pos_), then, if real_pos is given,
    setRealEEAgentPosition(real_pos): an init_pos away from the real position opens the step's gate from the first tick"""
    init_pos = scene["start"] if init_pos is None else init_pos
    planner.set_initial_position(init_pos)
    if real_pos is not None:
        planner.set_real_position(real_pos)
    return np.asarray(init_pos, dtype=np.float64)


def n_populations(planner):
    return int(getattr(planner, "P", 1))


def snapshot(planner, pop=None):
    """every getter the shadowing reads, as numpy arrays: one population; for a P-population planner population `pop`,
    or (pop=None) the list of every population's"""
    P = n_populations(planner)
    s = {}
    s["real_pos"], s["real_vel"], _ = [np.array(x) for x in planner.real_state()]
    s["real_known"], s["real_rot"] = [np.array(x) for x in planner.real_known()]
    s["paths"], s["n"] = [np.array(x) for x in planner.paths()]
    for k in ("agent_vel", "min_obs_dist", "rot_vecs", "known", "success", "costs"):
        s[k] = np.array(getattr(planner, k)())
    if P == 1:
        s["best_id"], s["best_type"] = planner.best_id(), planner.best_type()
        return s
    types, ids = [np.array(x) for x in planner.best()]
    s["best_id"], s["best_type"] = ids, types
    per = [{k: v[p] for k, v in s.items()} for p in range(P)]
    for q in per:
        q["best_id"], q["best_type"] = int(q["best_id"]), int(q["best_type"])
    return per if pop is None else per[pop]


def check_evaluate(A, st, scene, pre, costs, best, agents):
    """CfManager::evaluateAgents on the rollout in `pre`: every sampled agent's cost; the selected index too when all
    agents are sampled and the argmin / hysteresis are decided (counted in st.selections). Two agents' fp64 costs are
    known to be the same bits when their inputs are (the same path and min_obs_dist). Two costs the reference computed
    with bound 0 and equal value are taken as a tie too (the all-zero costs of tests/hp_select.py need this): that is safe
    because each of them has just been held to the planner's cost with bound 0 by st.check above -- a planner whose
    operation order rounds where the reference's does not fails there, before the selection is looked at"""
    N = int(scene["n_agents"])
    qc = {}
    for i in agents:
        def one(i=i):
            q = hp.agent_cost(A, pre["paths"][i, :pre["n"][i]], pre["min_obs_dist"][i], scene["goal"],
                              scene["approach_dist"], scene["cost_gains"], scene["ws_limits"])
            st.check("cost[%d]" % i, q, costs[i])
            qc[i] = q
        st.run(A, one)
    if len(qc) == N:
        keys = [("exact", qc[i].v) if qc[i].e == 0.0 else
                (pre["paths"][i, :pre["n"][i]].tobytes(), float(pre["min_obs_dist"][i])) for i in range(N)]

        def sel():
            st.expect("best index", hp.select_best(A, [qc[i] for i in range(N)], pre["best_id"], keys), best)
        if st.run(A, sel):
            st.selections += 1


def check_real(A, st, scene, pre, post, init_pos, obs_rows, best):
    """RealCfAgent::cfPlanner, one step (B/src/cf_agent.cpp:343-366) with the heuristic and random vectors of the agent
    selected this tick, from the previous real state"""
    def real():
        a = hp.Agent(A, pre["real_pos"], pre["real_vel"], scene["goal"], init_pos, pre["real_known"], pre["real_rot"],
                     atype=hp.REAL, **_params(scene))
        hp.step(A, a, hp.obstacles_from_rows(A, obs_rows), _gains(scene, best), scene["dt"], track_min=False,
                htype=post["best_type"], hrand=[A.v3(r) for r in scene["random_vecs"][best]])
        st.check_vec("real pos", a.latest, post["real_pos"])
        st.check_vec("real vel", a.vel, post["real_vel"])
        for k in range(len(a.known)):
            st.expect("real known[%d]" % k, a.known[k], bool(post["real_known"][k]))
            if a.known[k] and not pre["real_known"][k]:
                st.check_vec("real rot[%d]" % k, a.rot[k], post["real_rot"][k])
    st.run(A, real)


def _reference_rollout(A, scene, i, pos, vel, known, rot_i, obs_rows, init_pos, memo):
    """the reference's rollout of agent i from exact inputs: (agent, ran). memo: a dict shared between planners that are
    shadowed on the same scene -- the reference is a function of the inputs' bits and the policy's two parameters alone,
    so it is computed once per distinct input (a rollout that is undecidable raises again, the decided branches return)"""
    def compute():
        a = hp.Agent(A, pos, (0.0, 0.0, 0.0), scene["goal"], init_pos, known, rot_i, atype=agent_types(scene)[i],
                     rand_vecs=scene["random_vecs"][i], **_params(scene))
        hp.set_velocity(A, a, vel)
        own = hp.obstacles_from_rows(A, obs_rows, radii=scene["obstacles"][:, 6])
        ran = hp.prediction(A, a, own, _gains(scene, i), scene["dt"], int(scene["max_prediction_steps"]))
        return a, ran
    if memo is None:
        return compute()
    prm = _params(scene)
    key = (A.eps, A.exact_divsqrt, agent_types(scene)[i], int(scene["max_prediction_steps"])) + tuple(
        np.ascontiguousarray(x, dtype=np.float64).tobytes() for x in (
            pos, vel, np.asarray(known, dtype=bool), rot_i, obs_rows, init_pos, scene["goal"], scene["random_vecs"][i],
            scene["obstacles"][:, 6], _gains(scene, i), scene["dt"], [prm[k] for k in sorted(prm)]))
    if key not in memo:
        try:
            memo[key] = compute() + (dict(A.seen),)
        except hp.Undecidable as e:
            memo[key] = e
    if isinstance(memo[key], hp.Undecidable):
        raise memo[key]
    a, ran, seen = memo[key]
    A.seen = {k: set(v) for k, v in seen.items()}
    return a, ran


def check_rollouts(A, st, scene, pos, vel, known, pre_rot, pre_success, post, obs_rows, init_pos, agents, memo=None):
    """resetEEAgents(pos, vel, obstacles) with the real agent's known flags (B/src/cf_manager.cpp:246-255), then every
    sampled agent's cfPrediction to its guard (capacity max_prediction_steps, B/src/cf_agent.cpp:302-341); its private
    obstacle copy keeps the radii it was constructed with (B/src/cf_agent.cpp:63-70). memo: see _reference_rollout"""
    for i in agents:
        def roll(i=i):
            a, ran = _reference_rollout(A, scene, i, pos, vel, known, pre_rot[i], obs_rows, init_pos, memo)
            n = int(post["n"][i])
            st.expect("n_points[%d]" % i, len(a.path), n)
            for k in range(1, min(len(a.path), n)):
                st.check_vec("path[%d][%d]" % (i, k), a.path[k], post["paths"][i, k])
            st.check_vec("vel[%d]" % i, a.vel, post["agent_vel"][i])
            st.check("min_obs_dist[%d]" % i, a.min_obs_dist, post["min_obs_dist"][i])
            st.expect("success[%d]" % i, a.reached_goal if ran else bool(pre_success[i]), bool(post["success"][i]))
            for k in range(len(a.known)):
                st.expect("known[%d][%d]" % (i, k), a.known[k], bool(post["known"][i, k]))
                if a.known[k] and not known[k]:
                    st.check_vec("rot[%d][%d]" % (i, k), a.rot[k], post["rot_vecs"][i, k])
        st.run(A, roll)


def coupled_rows(obs_rows, pre, coupling):
    """the obstacle rows a population of a coupled handle actually sees this tick: for each coupled population p
    (coupling {p: (src_pop, radius)}), the trailing row is the source population's previous real position, velocity 0,
    the coupling radius (shard.DualArmCoupling, include/pmaf.h "peer mailboxes")"""
    out = np.array(obs_rows, dtype=np.float64, copy=True)
    for p, (src, radius) in (coupling or {}).items():
        out[p, -1, 0:3] = pre[src]["real_pos"]
        out[p, -1, 3:6] = 0.0
        out[p, -1, 6] = radius
    return out


def shadow_tick(planner, scene, obs_rows, init_pos, A, st, agents=None, rollouts=None, coupling=None, eval_agents=None,
                eval_stats=None):
    """one planCallback tick (evaluate, move the real agent, reset, roll out; B/src/panda_bimanual_control.cpp:336-352)
    shadowed: costs from the previous paths, the real agent's step from the previous real state with the agent selected
    this tick, every sampled agent's rollout from the new real state. rollouts: the rollout checker (check_rollouts, or
    tests/hp_anchored.py's walker). scene a list of P scene dicts: a P-population planner, every population shadowed
    (obs_rows [P, M, 7], init_pos [P, 3], coupling as in coupled_rows); returns the per-population best indices.
    eval_agents: agents whose cost is compared IN ADDITION to those of `agents` (whose rollouts are checked), into
    eval_stats (default: st) -- a separate Stats keeps the undecidable share of st what it was; "all" compares every
    agent's cost and therefore the selected index too."""
    rollouts = check_rollouts if rollouts is None else rollouts
    if isinstance(scene, dict):
        agents = list(range(int(scene["n_agents"]))) if agents is None else list(agents)
        est = st if eval_stats is None else eval_stats
        obs_rows = np.asarray(obs_rows, dtype=np.float64)
        pre = snapshot(planner)
        best = int(planner.tick(obs_rows, scene["dt"], scene["cost_gains"], scene["ws_limits"]))
        post = snapshot(planner)
        assert post["best_id"] == best + 1
        check_evaluate(A, st, scene, pre, post["costs"], best, agents)
        if eval_agents is not None:
            check_evaluate(A, est, scene, pre, post["costs"], best, _eval_agents(eval_agents, scene))
        check_real(A, st, scene, pre, post, init_pos, obs_rows, best)
        rollouts(A, st, scene, post["real_pos"], post["real_vel"], post["real_known"], pre["rot_vecs"],
                 pre["success"], post, obs_rows, init_pos, agents)
        return best
    scs = list(scene)
    P = len(scs)
    assert n_populations(planner) == P
    obs_rows = np.asarray(obs_rows, dtype=np.float64).reshape(P, -1, 7)
    init_pos = np.asarray(init_pos, dtype=np.float64).reshape(P, 3)
    pre = snapshot(planner)
    s0 = scs[0]
    best = [int(b) for b in np.ravel(planner.tick(obs_rows, s0["dt"], s0["cost_gains"], s0["ws_limits"]))]
    post = snapshot(planner)
    rows = coupled_rows(obs_rows, pre, coupling)
    for p, sc in enumerate(scs):
        ag = list(range(int(sc["n_agents"]))) if agents is None else list(agents)
        assert post[p]["best_id"] == best[p] + 1, (p, post[p]["best_id"], best[p])
        check_evaluate(A, st, sc, pre[p], post[p]["costs"], best[p], ag)
        if eval_agents is not None:
            check_evaluate(A, st if eval_stats is None else eval_stats, sc, pre[p], post[p]["costs"], best[p],
                           _eval_agents(eval_agents, sc))
        check_real(A, st, sc, pre[p], post[p], init_pos[p], rows[p], best[p])
        _call_rollouts(rollouts, A, st, sc, pre[p], post[p], rows[p], init_pos[p], ag, "pop %d " % p)
    return best


def _eval_agents(eval_agents, scene):
    return list(range(int(scene["n_agents"]))) if isinstance(eval_agents, str) and eval_agents == "all" else list(eval_agents)


def _call_rollouts(rollouts, A, st, sc, pre, post, rows, init_pos, agents, label):
    args = (A, st, sc, post["real_pos"], post["real_vel"], post["real_known"], pre["rot_vecs"], pre["success"], post,
            rows, init_pos, agents)
    if rollouts is check_rollouts:
        rollouts(*args)
    else:
        rollouts(*args, label=label)


def shadow_reset_rollout(planner, scene, pos, vel, obs_rows, init_pos, A, st, agents=None):
    """resetEEAgents(pos, vel, obstacles) + one rollout, shadowed"""
    agents = list(range(int(scene["n_agents"]))) if agents is None else list(agents)
    obs_rows = np.asarray(obs_rows, dtype=np.float64)
    pre = snapshot(planner)
    planner.reset_agents(pos, vel, obs_rows)
    planner.rollout()
    post = snapshot(planner)
    check_rollouts(A, st, scene, np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64),
                   pre["real_known"], pre["rot_vecs"], pre["success"], post, obs_rows, init_pos, agents)


def shadow_evaluate(planner, scene, A, st, agents=None):
    """evaluateAgents alone, shadowed"""
    agents = list(range(int(scene["n_agents"]))) if agents is None else list(agents)
    pre = snapshot(planner)
    best = int(planner.evaluate(scene["cost_gains"], scene["ws_limits"]))
    check_evaluate(A, st, scene, pre, np.array(planner.costs()), best, agents)
    return best


def shadow_steps(planner, scene, obs_rows, init_pos, A, st, n_calls, agents=None):
    """the synchronous stepping API: move_agents(obstacles, dt, steps=1) repeated (CfManager::moveAgents ->
    CfAgent::cfPlanner, B/src/cf_manager.cpp:274-291, B/src/cf_agent.cpp:278-300), each call shadowed from the
    handle's previous position, velocity, known flags, rotation vectors and min_obs_dist"""
    N = int(scene["n_agents"])
    types = agent_types(scene)
    prm = _params(scene)
    rv = scene["random_vecs"]
    agents = list(range(N)) if agents is None else list(agents)
    obs_rows = np.asarray(obs_rows, dtype=np.float64)
    for _ in range(n_calls):
        paths, n_pts = [np.array(x) for x in planner.paths()]
        vel, mod, rot, known = [np.array(x) for x in (planner.agent_vel(), planner.min_obs_dist(), planner.rot_vecs(),
                                                     planner.known())]
        planner.move_agents(obs_rows, scene["dt"], 1)
        paths2, n2 = [np.array(x) for x in planner.paths()]
        vel2, mod2, rot2, known2 = [np.array(x) for x in (planner.agent_vel(), planner.min_obs_dist(), planner.rot_vecs(),
                                                         planner.known())]
        for i in agents:
            def one(i=i):
                a = hp.Agent(A, paths[i, n_pts[i] - 1], vel[i], scene["goal"], init_pos, known[i], rot[i],
                             atype=types[i], rand_vecs=rv[i], min_obs_dist=mod[i], **prm)
                hp.step(A, a, hp.obstacles_from_rows(A, obs_rows), _gains(scene, i), scene["dt"])
                st.expect("n_points[%d]" % i, int(n_pts[i]) + 1, int(n2[i]))
                st.check_vec("pos[%d]" % i, a.latest, paths2[i, n2[i] - 1])
                st.check_vec("vel[%d]" % i, a.vel, vel2[i])
                st.check("min_obs_dist[%d]" % i, a.min_obs_dist, mod2[i])
                for k in range(len(a.known)):
                    st.expect("known[%d][%d]" % (i, k), a.known[k], bool(known2[i, k]))
                    if a.known[k] and not known[i, k]:
                        st.check_vec("rot[%d][%d]" % (i, k), a.rot[k], rot2[i, k])
            st.run(A, one)


def shadow_link_force(planner, scene, link_pos, k_r, obs_rows, A, st):
    out = np.asarray(planner.link_force(link_pos, k_r, obs_rows))
    for j in range(len(link_pos)):
        def one(j=j):
            q = hp.body_force(A, link_pos[j], k_r[j], hp.obstacles_from_rows(A, obs_rows),
                              shell=scene["detect_shell_rad"], rad=scene.get("radius", 0.05))
            st.check_vec("link_force[%d]" % j, q, out[j])
        st.run(A, one)


def shadow_eval_obstacle_distance(planner, scene, obs_rows, A, st):
    paths, n_pts = [np.array(x) for x in planner.paths()]
    out = np.asarray(planner.eval_obstacle_distance(obs_rows))
    for i in range(int(scene["n_agents"])):
        def one(i=i):
            q = hp.eval_obstacle_distance(A, paths[i, n_pts[i] - 1], hp.obstacles_from_rows(A, obs_rows),
                                          shell=scene["detect_shell_rad"], rad=scene.get("radius", 0.05))
            st.check("eval_obstacle_distance[%d]" % i, q, out[i])
        st.run(A, one)
