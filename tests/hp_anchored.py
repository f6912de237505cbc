"""Anchored rollout shadow: every step of a planner's whole returned rollout against the high-precision reference
(tests/hp_reference.py), each step started from the planner's OWN state at that step, so the bound never compounds
along the horizon (hp_shadow.check_rollouts carries it from the reset state and stops deciding within a few dozen
steps on real scenes).

Per step k of agent i the state is
  position  p_k  = the returned path point: an exact double, bound 0;
  velocity  v_k  in a Euclidean ball B(c_k, r_k) (no per-step velocity leaves a planner: see Ball);
  the known flags and rotation vectors, latched by the walk itself and anchored to the returned values;
  the agent's private obstacle copy: the tick's rows advanced k times by hp.predict_obstacles, with the radii the agent
  was constructed with (B/src/cf_agent.cpp:63-70).
Every step runs the cheap part of the step (gate, skip tests, floored distances, running min_obs_dist, shell/latch and
the latched rotation vector: B/src/cf_agent.cpp:72-108, 315-317) and the ball recursion. The full force check --
hp.step from (p_k, v_k), p_{k+1} within its bound, every branch decided on the reference's side -- runs on a seeded
subset of the steps, on every latch step and on the last 3 steps. At the end: the guard ends the walk exactly at the
returned n_points, reached_goal_ / success, min_obs_dist, the final known flags, and the last ball contains the
returned agent velocity.

Undecidable steps: a full check whose branches the bounds cannot decide is counted and skipped (the ball goes on: it
depends on positions only). An undecidable velocity clamp, latch, gate or skip decision ends that agent's walk (the
velocity, known flags and running minimum after it are not determined), and is counted too.
"""
import math

import numpy as np

import hp_reference as hp
import hp_shadow as sh

_MP = hp._MP
# |acc| after the clamp of updatePositionAndVelocity (B/src/cf_agent.cpp:253-268): fl(|a|) > 13 scales by
# fl(13 / fl(|a|)), so |a| <= 13 (1 + 6 eps); otherwise fl(|a|) <= 13, so |a| <= 13 / (1 - 3 eps). 2^-40 covers both for
# eps <= 2^-51.
A_MAX = 13.0 * (1.0 + 2.0 ** -40)
_INFL = 1.0 + 2.0 ** -45            # the rounding of the radius arithmetic itself (done in doubles)
_MPREL = 2.0 ** -100                # relative rounding of one centre update at hp.PREC = 113 bits


def _mnorm(c):
    return _MP.sqrt(sum(x * x for x in c))


def step_rounding(eps, dt, p_norm, v_norm):
    """(dp, dv): Euclidean bounds on the rounding of one updatePositionAndVelocity given |p_k| and a bound on |v_k|.

    With a the planner's (fp64) acceleration and every operation of relative error <= eps, per component i:
      w_i  = fl(dt v_i):                          |w_i - dt v_i|       <= eps dt |v_i|   (0 when fused into the sum)
      h_i  = 0.5, dt, dt, a_i multiplied in any order, at most three roundings (the 0.5 scaling is exact):
                                                  |h_i - dt^2 a_i / 2| <= 3.01 eps dt^2 |a_i| / 2
      p_i + h_i + w_i in ANY association, fused or not, at most two more roundings, each <= eps times a partial sum:
                                                  <= 2.01 eps (|p_i| + |h_i| + |w_i|)
    so   |dp_i| <= eps (3.02 dt |v_i| + 5.05 dt^2 |a_i| / 2 + 2.01 |p_i|),
    and for u = fl(v + fl(dt a)) or fma(dt, a, v):
         |dv_i| <= eps dt |a_i| + eps (|v_i| + (1 + eps) dt |a_i|) <= eps (2.01 dt |a_i| + 1.01 |v_i|).
    The Euclidean norm of a vector of such component bounds is at most the same combination of the vectors' norms
    (triangle inequality), with |a| <= A_MAX."""
    return comp_rounding(eps, dt, p_norm, v_norm, A_MAX)


def comp_rounding(eps, dt, p, v, a):
    """step_rounding's bounds for one component, given |p_i| and bounds on |v_i| and |a_i|"""
    dp = eps * (3.02 * dt * v + 5.05 * 0.5 * dt * dt * a + 2.01 * p)
    dv = eps * (2.01 * dt * a + 1.01 * v)
    return dp * _INFL, dv * _INFL


def second_difference(A, p_prev, p_k, acc_prev, acc_k, vel_prev, vel_k, dt):
    """p_{k+1} predicted without the velocity, for a step k whose previous step did not clamp the velocity:
    with p_k - p_{k-1} = dt v_{k-1} + dt^2 a_{k-1} / 2 + dp_{k-1}, v_k = v_{k-1} + dt a_{k-1} + dv_{k-1} and
    p_{k+1} = p_k + dt v_k + dt^2 a_k / 2 + dp_k,
        p_{k+1} = 2 p_k - p_{k-1} + dt^2 (a_{k-1} + a_k) / 2 + dt dv_{k-1} + dp_k - dp_{k-1}.
    The accelerations are the reference's (acc_prev, acc_k: carried, their bounds hold the velocity ball's effect on
    the force, which dt^2 / 2 makes small); the roundings are comp_rounding's. The ball's radius -- the sum of every
    earlier step's rounding, 2 |dp| / dt each -- drops out: the bound stays a few ulp of p over any horizon, where the
    direct check from the ball carries dt r."""
    h = hp.MPF(dt) * hp.MPF(dt) / 2
    out = []
    for i in range(3):
        c = 2 * hp.MPF(float(p_k[i])) - hp.MPF(float(p_prev[i])) + h * (acc_prev[i].v + acc_k[i].v)
        ap, ak = abs(float(acc_prev[i].v)) + acc_prev[i].e, abs(float(acc_k[i].v)) + acc_k[i].e
        vp, vk = abs(float(vel_prev[i].v)) + vel_prev[i].e, abs(float(vel_k[i].v)) + vel_k[i].e
        dp0, dv0 = comp_rounding(A.eps, dt, abs(float(p_prev[i])), vp, ap)
        dp1, _ = comp_rounding(A.eps, dt, abs(float(p_k[i])), vk, ak)
        e = (float(h) * (acc_prev[i].e + acc_k[i].e) + dt * dv0 + dp0 + dp1 + 2.0 ** -100 * abs(float(c))) * _INFL
        out.append(hp.Q(c, e))
    return tuple(out)


class Ball:
    """the enclosure of one agent's velocity: |v - c| <= r (c at hp.PREC bits, r a double).

    The step is p_{k+1} = p_k + dt v_k + dt^2 a_k / 2 + dp and u = v_k + dt a_k + dv, v_{k+1} = clamp(u) (B/src/
    cf_agent.cpp:253-268). Eliminating a_k: u = 2 (p_{k+1} - p_k) / dt - v_k - 2 dp / dt + dv, so with v_k in B(c, r)
      u in B(2 (p_{k+1} - p_k) / dt - c,  r + 2 |dp| / dt + |dv|).
    The clamp, when decided, is the projection onto the ball of radius velocity_max, which is 1-Lipschitz: the radius
    carries over and only the clamp's own rounding is added -- fl(|u|) (three products and two sums: 3 eps relative,
    halved by the root, plus the root's eps), the quotient and the product: u (vel_max / |u|) (1 + theta) with
    |theta| <= 4.5 eps, and where fl(|u|) > vel_max >= |u| the projection is u itself, at most 3 eps vel_max away.
    8 eps vel_max covers both. The decision itself compares |c| +- (r + 3.01 eps (|c| + r)) with vel_max."""

    def __init__(self, centre, radius):
        self.c = tuple(centre)
        self.r = float(radius)
        self.clamped = False           # the step that made this ball clamped the velocity

    @classmethod
    def of(cls, qv):
        """the ball around a carried vector (tuple of hp.Q)"""
        return cls([q.v for q in qv], math.sqrt(sum(q.e * q.e for q in qv)) * _INFL)

    def q(self):
        """as carried quantities: every component of v lies within r of the centre's"""
        return tuple(hp.Q(x, self.r) for x in self.c)

    def contains(self, x):
        return float(_mnorm([hp.MPF(float(t)) - c for t, c in zip(x, self.c)])) <= self.r

    def ratio(self, x):
        d = float(_mnorm([hp.MPF(float(t)) - c for t, c in zip(x, self.c)]))
        return 0.0 if d == 0 else (math.inf if self.r == 0 else d / self.r)

    def advance(self, A, p0, p1, dt, vel_max):
        """the ball of v_{k+1} from exact p_k = p0, p_{k+1} = p1; records the vel_clamp decision; raises hp.Undecidable
        when the clamp is not decided"""
        cn = float(_mnorm(self.c))
        dp, dv = step_rounding(A.eps, dt, float(_mnorm([hp.MPF(float(t)) for t in p0])), cn + self.r)
        two_dt = 2 / hp.MPF(dt)
        u = tuple(two_dt * (hp.MPF(float(b)) - hp.MPF(float(a))) - c for a, b, c in zip(p0, p1, self.c))
        un = _mnorm(u)
        r = (self.r + 2.0 * dp / dt + dv + _MPREL * (float(un) + cn)) * _INFL
        nq = hp.Q(un, (r + 3.01 * A.eps * (float(un) + r)) * _INFL)
        if A.decide("vel_clamp", nq, ">", A.c(vel_max)):
            vm = hp.MPF(float(vel_max))
            b = Ball([vm * x / un for x in u], (r + 8.0 * A.eps * vel_max + _MPREL * vel_max) * _INFL)
            b.clamped = True
            return b
        return Ball(u, r)


# ---------------------------------------------------------------------------------------------------------------------
# the cheap part of the step
# ---------------------------------------------------------------------------------------------------------------------
def latch_step(A, a, obstacles, htype, hrand):
    """gate (B/src/cf_agent.cpp:315-317), then CfAgent::circForce's per-obstacle skip tests, floored distance, running
    minimum and shell/latch (:72-108) -- everything of the step the state after it depends on except the force. The
    running minimum is carried as an enclosure: fp64 min() of values each within e_j of v_j is within max(e_j) of
    min(v_j), whichever way close values compare. Returns the obstacles latched (known set, rotation vector computed)."""
    latched = []
    if not hp.gate_open(A, a):
        return latched
    p = a.latest
    goal_vec = A.vsub(a.goal, p)
    ng = A.normalized(goal_vec)
    for i in range(len(obstacles) - 1):
        o = obstacles[i]
        ro = A.vsub(o.pos, p)
        if A.decide("skip_dir", A.dot(A.normalized(ro), ng), "<", A.c(-0.01)):
            if A.decide("skip_vel", A.dot(ro, A.vsub(a.vel, o.vel)), "<", A.c(-0.01)):
                continue
        dist = hp._floored_dist(A, p, o, a.rad)
        m = a.min_obs_dist
        if dist.v < m.v:
            a.min_obs_dist = hp.Q(dist.v, max(dist.e, m.e))
        elif dist.e > m.e:
            a.min_obs_dist = hp.Q(m.v, max(dist.e, m.e))
        if A.decide("shell", dist, "<", a.shell):
            A.note("known", a.known[i])
            if not a.known[i]:
                a.rot[i] = hp.rotation_vector(A, htype, p, a.goal, obstacles, i, hrand)
                a.known[i] = True
                latched.append(i)
    return latched


def full_steps(n_steps, frac, seed):
    """the seeded subset of steps 0..n_steps-1 that get the full force check (frac >= 1: every step); each sampled step
    comes with the step before it, for the second-difference check"""
    if frac >= 1.0:
        return set(range(n_steps))
    rng = np.random.default_rng(seed)
    ks = np.nonzero(rng.random(n_steps) < frac / 2)[0]
    return set(ks.tolist()) | set((ks[ks > 0] - 1).tolist())


class Walk:
    """per-case extras of the anchored walks, printed with the Stats report"""

    def __init__(self):
        self.walks = 0
        self.ended = {}
        self.steps = 0
        self.full = 0
        self.latches = []          # (agent, step, obstacle)
        self.max_radius = 0.0
        self.max_pos_bound = 0.0
        self.worst_vel = 0.0
        self.horizon = 0
        self.sd_checks = 0
        self.max_sd_bound = 0.0

    def line(self):
        return ("    anchored: %d walks, %d steps (horizon up to %d), %d full checks, %d latches, walks ended early %s, "
                "max ball radius %.3g m/s, max position bound %.3g m (second difference: %d checks, max bound %.3g m), "
                "final velocity / radius <= %.3g" % (
                    self.walks, self.steps, self.horizon, self.full, len(self.latches), self.ended or "{}",
                    self.max_radius, self.max_pos_bound, self.sd_checks, self.max_sd_bound, self.worst_vel))


def _walk_stats(st):
    if not hasattr(st, "walk"):
        st.walk = Walk()
        st.notes.append(st.walk.line)
    return st.walk


def walk_agent(A, st, scene, i, pos, vel, known, rot0, pre_success, post, obs_rows, init_pos, *, frac=1.0, seed=0,
               label=""):
    """resetEEAgents(pos, vel, obstacles) with the real agent's known flags (B/src/cf_manager.cpp:246-255), then agent
    i's returned rollout walked step by step (module docstring)"""
    W = _walk_stats(st)
    types = sh.agent_types(scene)
    radii0 = scene["obstacles"][:, 6]
    cap = int(scene["max_prediction_steps"])
    dt = float(scene["dt"])
    vmax = float(scene["velocity_max"])
    gains = sh._gains(scene, i)
    prm = sh._params(scene)
    n = int(post["n"][i])
    path = post["paths"][i]
    tag = "%sagent %d" % (label, i)
    W.walks += 1
    W.horizon = max(W.horizon, n - 1)

    # the walking state: exact position, velocity ball, latched flags / anchored rotation vectors, running minimum
    a = hp.Agent(A, pos, (0.0, 0.0, 0.0), scene["goal"], init_pos, known, rot0, atype=types[i],
                 rand_vecs=scene["random_vecs"][i], **prm)
    hrand = a.rand
    A.seen = {}
    try:
        hp.set_velocity(A, a, vel)
        ball = Ball.of(a.vel)
    except hp.Undecidable:
        # |vel| within rounding of velocity_max (the real agent's own clamp): clamped or not, the result is within
        # fl(|vel|) - vel_max <= 3 eps |vel| of vel, plus the clamp's rounding (Ball: 8 eps vel_max)
        ball = Ball([hp.MPF(float(x)) for x in vel], 16.0 * A.eps * max(vmax, float(np.linalg.norm(vel))))
    st.merge_seen(A.seen)
    own = hp.obstacles_from_rows(A, obs_rows, radii=radii0)
    full = full_steps(max(n - 1, 0), frac, seed * 1000003 + i)
    full.update(range(max(n - 4, 0), n - 1))
    fails0 = len(st.failures)
    prev = {}                       # the last full step's k, acceleration and velocity (second-difference check)

    k = 0
    while True:
        p_k = path[k]
        a.path = [A.v3(p_k)]
        a.vel = ball.q()
        # the rollout guard on p_k (B/src/cf_agent.cpp:313): true before every returned step, false (or full) at n - 1
        A.seen = {}
        try:
            g = A.decide("guard", hp.dist_from_goal(A, a), ">", A.c(0.1))
        except hp.Undecidable as e:
            return _end(st, W, str(e))
        st.merge_seen(A.seen)
        if k == n - 1:
            st.expect("%s guard ends the walk at n_points %d" % (tag, n), False, g and n < cap)
            break
        if not (g and k + 1 < cap):
            st.expect("%s guard at step %d (n_points %d)" % (tag, k, n), True, False)
            break
        # the state before the step, for the full check
        known_k, rot_k = list(a.known), list(a.rot)
        # cheap part: gate, skips, minimum, latch (rotation vector on a latch)
        A.seen = {}
        try:
            latched = latch_step(A, a, own, types[i], hrand)
        except hp.Undecidable as e:
            return _end(st, W, "latch " + str(e))
        st.merge_seen(A.seen)
        for j in latched:
            W.latches.append((i, k, j))
            st.check_vec("%s rot[%d] latched at step %d" % (tag, j, k), a.rot[j], post["rot_vecs"][i, j])
            a.rot[j] = A.v3(post["rot_vecs"][i, j])          # anchored for the later steps
        # the ball of v_{k+1}
        A.seen = {}
        try:
            nxt = ball.advance(A, p_k, path[k + 1], dt, vmax)
        except hp.Undecidable as e:
            return _end(st, W, str(e))
        st.merge_seen(A.seen)
        # the full force check
        if k in full or latched:
            W.full += 1

            def one(k=k, known_k=known_k, rot_k=rot_k, nxt=nxt):
                b = hp.Agent(A, p_k, (0.0, 0.0, 0.0), scene["goal"], init_pos, known_k, [(0.0, 0.0, 0.0)] * len(rot_k),
                             atype=types[i], rand_vecs=None, **prm)
                b.vel, b.rot, b.rand = ball.q(), list(rot_k), hrand
                hp.step(A, b, own, gains, dt, track_min=False)
                st.check_vec("%s path[%d]" % (tag, k + 1), b.latest, path[k + 1])
                W.max_pos_bound = max(W.max_pos_bound, max(q.e for q in b.latest))
                if prev.get("k") == k - 1 and not ball.clamped:
                    q2 = second_difference(A, path[k - 1], p_k, prev["acc"], b.acc, prev["vel"], ball.q(), dt)
                    st.check_vec("%s path[%d] second difference" % (tag, k + 1), q2, path[k + 1])
                    W.sd_checks += 1
                    W.max_sd_bound = max(W.max_sd_bound, max(q.e for q in q2))
                prev.update(k=k, acc=b.acc, vel=ball.q())
                # the next ball and the reference's velocity must meet
                gap = float(_mnorm([q.v - c for q, c in zip(b.vel, nxt.c)]))
                ve = math.sqrt(sum(q.e * q.e for q in b.vel))
                st.components += 1
                if gap > (ve + nxt.r) * sh.BOUND_FACTOR:
                    st.failures.append("%s vel[%d]: derived ball %.3g m/s from the reference (bound %.3g)"
                                       % (tag, k + 1, gap, ve + nxt.r))
                for j in range(len(b.known)):
                    if b.known[j] != a.known[j]:
                        st.failures.append("%s known[%d] at step %d: full step %r, latch walk %r"
                                           % (tag, j, k, b.known[j], a.known[j]))
            st.run(A, one)                             # its own sample: counted, skipped when undecidable
        hp.predict_obstacles(A, own, dt)
        ball = nxt
        W.steps += 1
        W.max_radius = max(W.max_radius, ball.r)
        k += 1

    # the end of the walk
    A.seen = {}
    try:
        ran = n > 1
        # reached_goal_ after the loop (B/src/cf_agent.cpp:330-335)
        reached = A.decide("reached", hp.dist_from_goal(A, a), "<", A.c(0.100001)) if ran else None
    except hp.Undecidable as e:
        return _end(st, W, str(e))
    st.merge_seen(A.seen)
    st.expect("%s success" % tag, reached if ran else bool(pre_success[i]), bool(post["success"][i]))
    st.check("%s min_obs_dist" % tag, a.min_obs_dist, post["min_obs_dist"][i])
    for j in range(len(a.known)):
        st.expect("%s known[%d]" % (tag, j), a.known[j], bool(post["known"][i, j]))
    r = ball.ratio(post["agent_vel"][i])
    W.worst_vel = max(W.worst_vel, r)
    st.components += 1
    if r > sh.BOUND_FACTOR:
        st.failures.append("%s agent_vel %r outside the last ball (|v - c| / r = %.3g, r = %.3g)"
                           % (tag, list(post["agent_vel"][i]), r, ball.r))
    st.compared += 1
    return len(st.failures) == fails0


def _end(st, W, why):
    st.undecidable += 1
    key = "walk ended: " + why
    st.undecided_at[key] = st.undecided_at.get(key, 0) + 1
    W.ended[why] = W.ended.get(why, 0) + 1
    return None


def walk_rollouts(A, st, scene, pos, vel, known, pre_rot, pre_success, post, obs_rows, init_pos, agents, *, frac=1.0,
                  seed=0, label=""):
    """hp_shadow.check_rollouts' signature: every sampled agent's returned rollout walked (walk_agent)"""
    for i in agents:
        walk_agent(A, st, scene, i, pos, vel, known, pre_rot[i], pre_success, post, obs_rows, init_pos, frac=frac,
                   seed=seed, label=label)


def walker(frac=1.0, seed=0):
    """a rollout checker for hp_shadow.shadow_tick(..., rollouts=walker(...))"""
    def check(A, st, scene, pos, vel, known, pre_rot, pre_success, post, obs_rows, init_pos, agents, label=""):
        walk_rollouts(A, st, scene, pos, vel, known, pre_rot, pre_success, post, obs_rows, init_pos, agents, frac=frac,
                      seed=seed, label=label)
    return check
