"""Independent high-precision reference of the planner step, with a running rounding-error bound.

TEST INFRASTRUCTURE ONLY. A second restatement of the reference planner, written from the reference's equations
(B/ = the reference's src/bimanual_planning_ros/; every function cites the lines it follows) and NOT from
oracle/pmaf_oracle.c: it imports neither oracle/ nor the package's ctypes layer (tests/test_hp_reference.py checks
this with `ast`), and it does not follow the oracle's evaluation order.

Arithmetic: mpmath at PREC bits. Every quantity is a pair Q(v, e): v the high-precision value of the expression, e an
absolute bound on how far an fp64 evaluation of the same expression, under an arithmetic policy whose every operation
has relative error <= eps, can be from v. Inputs are exact doubles (e = 0). Each operation propagates its inputs'
bounds through its derivatives (rigorously: products keep the e_a e_b term, quotients and roots use the worst end of
the input interval) and adds eps * |result|. An operation whose inputs carry e = 0 and whose result is exactly a double
adds nothing when the policy rounds correctly (+ - * always; / and sqrt under the strict policies): IEEE then returns
those bits, which is what decides the exact-tie scenes. Sums of three or more terms take a bound that holds for every
association, so one reference serves both dot-product associations and the tree-shaped force sum of the contracted
policy.

Decisions: every branch of the step compares two carried quantities. The comparison is decided when the values'
gap exceeds the sum of their bounds (or both bounds are 0: the fp64 operands are then the exact values); otherwise
the evaluation raises Undecidable and the sample is not compared. Each decided branch outcome is recorded in
Arith.seen, so a test can show that both sides of every branch were exercised.
"""
import math

from mpmath.ctx_mp import MPContext

PREC = 113
U = 2.0 ** -53                 # unit roundoff of IEEE double: MATH_XACT, MATH_IEEE
# MATH_FAST / MATH_FMA: csrc/pmaf_device.hpp documents the v_rcp_f64 / v_rsq_f64 seeds plus two Newton (Goldschmidt)
# iterations as "1-2 ulp per operation". 2 ulp of a result r is at most 2 * 2^-52 |r|. Measured since
# (tests/test_hard_rounding_gpu.py, constructed hard cases + 1e6 random operands): at most 0.53 of this per operation.
EPS_FAST = 2.0 ** -51
# the restated exp (glibc's algorithm, 0.511 ulp; test_device_arithmetic_is_ieee_exact holds the kernels' exp to it bit
# for bit): 1 ulp <= 2^-52 relative
EPS_EXP = 2.0 ** -52
_INFL = 1.0 + 2.0 ** -45       # covers the rounding of the bound arithmetic itself (done in doubles)

POLICIES = {
    # name: (per-operation relative error, whether / and sqrt are correctly rounded)
    "xact": (U, True),
    "ieee": (U, True),
    "fast": (EPS_FAST, False),
    "fma": (EPS_FAST, False),
}

# agent types, CfAgent::Type (B/include/bimanual_planning_ros/cf_agent.h:59-68)
REAL, GOAL, OBSTACLE, GOAL_OBSTACLE, VEL, RANDOM, HAD = range(7)

# every branch the step, the rollout guard, the evaluation and the stepping API decide (keys of Arith.seen). Not listed:
# attractorForceScaling's no_close_obs return (:212-214) is recorded as "scale_none" but cannot be taken -- the scaling is
# only called when circForce added a force, i.e. some field obstacle's floored distance was inside the shell, and the
# scaling's loop finds that same distance
BRANCHES = (
    "skip_dir", "skip_vel", "floor", "min_obs", "shell", "known", "vel_norm", "degenerate", "closest_other",
    "force_gate", "scale_closest", "scale_zero", "acc_clamp", "vel_clamp", "setvel_clamp",
    "gate", "guard", "reached", "penalty", "goal_cost", "ws", "argmin", "hysteresis", "eod_min",
)

_MP = MPContext()
_MP.prec = PREC
MPF = _MP.mpf


class Undecidable(Exception):
    """a branch (or a division / root) whose outcome the carried bounds cannot decide"""


class Q:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = v
        self.e = e

    def __repr__(self):
        return "Q(%s +- %.3g)" % (_MP.nstr(self.v, 20), self.e)

    @property
    def f(self):
        return float(self.v)


def _is_double(v):
    return MPF(float(v)) == v


class Arith:
    """one arithmetic policy: the operations on carried quantities and the decision rule"""

    def __init__(self, policy="xact"):
        self.policy = policy
        self.eps, self.exact_divsqrt = POLICIES[policy]
        self.seen = {}            # branch -> set of decided outcomes of the current sample
        self.ONE = self.c(1.0)
        self.ZERO = self.c(0.0)

    # -- scalars --
    def c(self, x):
        return Q(MPF(float(x)), 0.0)

    def _round(self, v, eprop, exact_ok=True):
        """add the rounding of the operation that produced v from inputs with propagated bound eprop"""
        if eprop == 0.0 and exact_ok and _is_double(v):
            return Q(v, 0.0)
        a = abs(float(v))
        return Q(v, (eprop + self.eps * (a + eprop)) * _INFL)

    def add(self, a, b):
        return self._round(a.v + b.v, a.e + b.e)

    def sub(self, a, b):
        return self._round(a.v - b.v, a.e + b.e)

    def neg(self, a):
        return Q(-a.v, a.e)

    def mul(self, a, b):
        ep = abs(float(a.v)) * b.e + abs(float(b.v)) * a.e + a.e * b.e
        return self._round(a.v * b.v, ep)

    def div(self, a, b):
        bv = abs(float(b.v))
        if b.v == 0 or bv <= b.e:
            raise Undecidable("division by a quantity that may be 0")
        v = a.v / b.v
        ep = 0.0
        if a.e or b.e:
            ep = (a.e + abs(float(v)) * b.e) / ((bv - b.e) * (1.0 - 2.0 ** -50))
        return self._round(v, ep, self.exact_divsqrt)

    def sqrt(self, a):
        x = float(a.v)
        if a.v < 0 and -x > a.e:
            raise Undecidable("root of a negative quantity")
        v = _MP.sqrt(a.v) if a.v > 0 else MPF(0)
        ep = 0.0
        if a.e:
            s = float(v)
            ep = max(s - math.sqrt(max(x - a.e, 0.0)), math.sqrt(x + a.e) - s) * (1.0 + 2.0 ** -50) + 2.0 ** -1074
        return self._round(v, ep, self.exact_divsqrt)

    def exp(self, a):
        v = _MP.exp(a.v)
        ep = float(v) * math.expm1(a.e) * (1.0 + 2.0 ** -50) if a.e else 0.0
        r = abs(float(v))
        return Q(v, (ep + max(EPS_EXP, self.eps) * (r + ep)) * _INFL)

    def sum_any(self, terms):
        """fp64 sum of the terms in ANY association (first rounding of each partial sum bounded by eps times the sum of
        the absolute values of all terms, at most n - 1 partial sums)"""
        terms = list(terms)
        if not terms:
            return self.ZERO
        if len(terms) == 1:
            return terms[0]
        v = terms[0].v
        for t in terms[1:]:
            v = v + t.v
        ep = sum(t.e for t in terms)
        if ep == 0.0 and _partial_sums_are_doubles(terms):
            return Q(v, 0.0)
        tot = sum(abs(float(t.v)) + t.e for t in terms)
        return Q(v, (ep + self.eps * (len(terms) - 1) * tot + self.eps * (abs(float(v)) + ep)) * _INFL)

    # -- decisions --
    def decide(self, name, a, op, b):
        """a op b for op in '<', '<=', '>', '>=', '!=' on carried quantities; records the outcome under `name`"""
        gap = a.v - b.v
        if a.e or b.e:
            if abs(float(gap)) <= a.e + b.e:
                raise Undecidable(name)
        r = {"<": gap < 0, "<=": gap <= 0, ">": gap > 0, ">=": gap >= 0, "!=": gap != 0}[op]
        self.seen.setdefault(name, set()).add(bool(r))
        return bool(r)

    def note(self, name, outcome):
        """a branch on exact state (the known-latch)"""
        self.seen.setdefault(name, set()).add(bool(outcome))

    # -- 3-vectors (tuples of Q) --
    def v3(self, x):
        return tuple(self.c(t) for t in x)

    def vadd(self, a, b):
        return tuple(self.add(x, y) for x, y in zip(a, b))

    def vsub(self, a, b):
        return tuple(self.sub(x, y) for x, y in zip(a, b))

    def vscale(self, s, a):
        return tuple(self.mul(s, x) for x in a)

    def vdiv(self, a, s):
        return tuple(self.div(x, s) for x in a)

    def dot(self, a, b):
        """(a0 b0 + a1 b1) + a2 b2 or a0 b0 + (a1 b1 + a2 b2), fused or not: the bound holds for both associations"""
        return self.sum_any([self.mul(x, y) for x, y in zip(a, b)])

    def norm(self, a):
        if self.exact_divsqrt and all(x.e == 0.0 for x in a) and sum(x.v != 0 for x in a) <= 1:
            # an axis-aligned exact vector: sqrt(fl(x * x)) = |x| in IEEE arithmetic (no underflow at these scales)
            return Q(max(abs(x.v) for x in a), 0.0)
        return self.sqrt(self.dot(a, a))

    def normalized(self, a):
        """Eigen normalized(): a / sqrt(z) if z = squaredNorm > 0, else a unchanged"""
        z = self.dot(a, a)
        if not self.decide("normalize", z, ">", self.ZERO):
            return a
        return self.vdiv(a, self.sqrt(z))

    def cross(self, a, b):
        return (self.sub(self.mul(a[1], b[2]), self.mul(a[2], b[1])),
                self.sub(self.mul(a[2], b[0]), self.mul(a[0], b[2])),
                self.sub(self.mul(a[0], b[1]), self.mul(a[1], b[0])))

    def vsum_any(self, vecs):
        vecs = list(vecs)
        return tuple(self.sum_any([v[k] for v in vecs]) for k in range(3))

    def smax(self, name, a, b):
        """std::max(a, b) = (a < b) ? b : a"""
        return b if self.decide(name, a, "<", b) else a

    def smin(self, name, a, b):
        """std::min(a, b) = (b < a) ? b : a"""
        return b if self.decide(name, b, "<", a) else a


def _partial_sums_are_doubles(terms):
    """every sum of two or more of the terms (what any association can form) is a double; lists longer than four are
    not examined (conservatively: a rounding is charged)"""
    from itertools import combinations
    n = len(terms)
    if n > 4:
        return False
    for k in range(2, n + 1):
        for idx in combinations(range(n), k):
            s = terms[idx[0]].v
            for i in idx[1:]:
                s = s + terms[i].v
            if not _is_double(s):
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------------------------------------------------
class Obs:
    """Obstacle (B/include/bimanual_planning_ros/obstacle.h:16-40): position, velocity, radius"""
    __slots__ = ("pos", "vel", "rad")

    def __init__(self, pos, vel, rad):
        self.pos, self.vel, self.rad = pos, vel, rad


def obstacles_from_rows(A, rows, radii=None):
    """flat [n][7] rows (px,py,pz,vx,vy,vz,r) as exact quantities; radii overrides the radius column (an agent's private
    copy keeps the radii it was constructed with: CfAgent::setObstacles copies position and velocity only,
    B/src/cf_agent.cpp:63-70)"""
    out = []
    for i, r in enumerate(rows):
        rad = r[6] if radii is None else radii[i]
        out.append(Obs(A.v3(r[0:3]), A.v3(r[3:6]), A.c(rad)))
    return out


class Agent:
    """the CfAgent state one step reads and writes (B/include/bimanual_planning_ros/cf_agent.h:36-56)"""

    def __init__(self, A, pos, vel, goal, init_pos, known, rot, *, shell, mass, rad, vel_max, approach,
                 atype, rand_vecs=None, min_obs_dist=None):
        self.path = [A.v3(pos)]
        self.vel = A.v3(vel)
        self.goal = A.v3(goal)
        self.init_pos = A.v3(init_pos)
        self.known = [bool(k) for k in known]
        self.rot = [A.v3(r) for r in rot]
        self.shell, self.mass, self.rad = A.c(shell), A.c(mass), A.c(rad)
        self.vel_max, self.approach = A.c(vel_max), A.c(approach)
        self.type = int(atype)
        self.rand = [A.v3(r) for r in rand_vecs] if rand_vecs is not None else None
        self.min_obs_dist = A.c(shell if min_obs_dist is None else min_obs_dist)
        self.reached_goal = None
        self.force = A.v3((0.0, 0.0, 0.0))

    @property
    def latest(self):
        return self.path[-1]


def dist_from_goal(A, a):
    """CfAgent::getDistFromGoal (cf_agent.h:116-118): (g - p).norm()"""
    return A.norm(A.vsub(a.goal, a.latest))


# ---------------------------------------------------------------------------------------------------------------------
# heuristics: B/src/cf_agent.cpp:389-611
# ---------------------------------------------------------------------------------------------------------------------
def _closest_other(A, obstacles, oid):
    """nearest other field obstacle by centre distance, first minimum (B/src/cf_agent.cpp:434-446, 480-492)"""
    min_d = A.c(100.0)
    closest = 0
    for i in range(len(obstacles) - 1):
        if i != oid:
            d = A.norm(A.vsub(obstacles[oid].pos, obstacles[i].pos))
            if A.decide("closest_other", min_d, ">", d):
                min_d, closest = d, i
    return closest


def _degenerate(A, cur):
    """if (current.norm() < 1e-10) current << 0, 0, 1 (B/src/cf_agent.cpp:400-403, 510-513, 531-534)"""
    if A.decide("degenerate", A.norm(cur), "<", A.c(1e-10)):
        return A.v3((0.0, 0.0, 1.0))
    return cur


def current_vector(A, htype, p, rel_vel, goal, obstacles, oid, rot):
    """currentVector of each heuristic (B/src/cf_agent.cpp:389-406 goal, 414-426 obstacle, 463-475 goal-obstacle,
    520-537 velocity, 545-557 random, 585-597 had); agent_vel is the relative velocity circForce passes (:100-101)"""
    if htype == GOAL:
        goal_vec = A.vsub(goal, p)
        to_obs = A.normalized(A.vsub(obstacles[oid].pos, p))
        cur = A.vsub(goal_vec, A.vscale(A.dot(to_obs, goal_vec), to_obs))
        return A.normalized(_degenerate(A, cur))
    if htype == VEL:
        nvel = A.normalized(rel_vel)
        to_agent = A.normalized(A.vsub(obstacles[oid].pos, p))
        cur = A.vsub(nvel, A.vscale(A.dot(nvel, to_agent), to_agent))
        return A.normalized(_degenerate(A, cur))
    if htype in (OBSTACLE, GOAL_OBSTACLE, RANDOM, HAD):
        to_obs = A.normalized(A.vsub(obstacles[oid].pos, p))
        return A.normalized(A.cross(to_obs, rot[oid]))
    raise ValueError("agent type %d has no currentVector" % htype)


def rotation_vector(A, htype, p, goal, obstacles, oid, rand):
    """calculateRotationVector of each heuristic (B/src/cf_agent.cpp:408-412, 428-461, 477-518, 539-543, 559-566,
    599-611)"""
    if htype in (GOAL, VEL):
        return A.v3((0.0, 0.0, 1.0))
    if htype in (OBSTACLE, GOAL_OBSTACLE):
        if htype == OBSTACLE and len(obstacles) < 2:
            return A.v3((0.0, 0.0, 1.0))
        c = _closest_other(A, obstacles, oid)
        obstacle_vec = A.vsub(obstacles[c].pos, obstacles[oid].pos)
        to_obs = A.normalized(A.vsub(obstacles[oid].pos, p))
        obst_cur = A.vsub(A.vscale(A.dot(obstacle_vec, to_obs), to_obs), obstacle_vec)
        if htype == OBSTACLE:
            return A.normalized(A.cross(obst_cur, to_obs))
        goal_vec = A.vsub(goal, p)
        goal_cur = A.vsub(goal_vec, A.vscale(A.dot(to_obs, goal_vec), to_obs))
        cur = A.vadd(A.normalized(goal_cur), A.normalized(obst_cur))
        cur = A.normalized(_degenerate(A, cur))
        return A.normalized(A.cross(cur, to_obs))
    if htype == RANDOM:
        g = A.normalized(A.vsub(goal, p))
        return A.cross(g, rand[oid])                       # not normalised (:564)
    if htype == HAD:
        o = obstacles[oid].pos
        goal_vec = A.vsub(goal, p)
        rob_obs = A.vsub(o, p)
        gn = A.norm(goal_vec)
        s = A.div(A.dot(rob_obs, goal_vec), A.mul(gn, gn))  # pow(goal_vec.norm(), 2)
        gs = A.vscale(s, goal_vec)
        d = tuple(A.sum_any([p[k], gs[k], A.neg(o[k])]) for k in range(3))
        cr = A.cross(d, goal_vec)
        return A.vdiv(cr, A.norm(cr))                      # unguarded (:609)
    raise ValueError("agent type %d has no rotation vector" % htype)


# ---------------------------------------------------------------------------------------------------------------------
# forces: B/src/cf_agent.cpp:72-268
# ---------------------------------------------------------------------------------------------------------------------
def _floored_dist(A, p, o, rad):
    """max(|p - o| - (rad_ + r), 1e-5)"""
    d = A.sub(A.norm(A.vsub(o.pos, p)), A.add(rad, o.rad))
    return A.smax("floor", d, A.c(1e-5))


def circ_terms(A, a, obstacles, k_circ, track_min, htype, hrand):
    """CfAgent::circForce (B/src/cf_agent.cpp:72-108, track_min) and RealCfAgent::circForce (:110-144: no
    min_obs_dist_, heuristics of the best agent). Returns the non-zero per-obstacle terms in obstacle order."""
    p = a.latest
    goal_vec = A.vsub(a.goal, p)
    terms = []
    for i in range(len(obstacles) - 1):
        o = obstacles[i]
        ro = A.vsub(o.pos, p)
        rel_vel = A.vsub(a.vel, o.vel)
        if A.decide("skip_dir", A.dot(A.normalized(ro), A.normalized(goal_vec)), "<", A.c(-0.01)):
            if A.decide("skip_vel", A.dot(ro, rel_vel), "<", A.c(-0.01)):
                continue
        dist = _floored_dist(A, p, o, a.rad)
        if track_min and A.decide("min_obs", dist, "<", a.min_obs_dist):
            a.min_obs_dist = dist
        if A.decide("shell", dist, "<", a.shell):
            A.note("known", a.known[i])
            if not a.known[i]:
                a.rot[i] = rotation_vector(A, htype, p, a.goal, obstacles, i, hrand)
                a.known[i] = True
            vel_norm = A.norm(rel_vel)
            if A.decide("vel_norm", vel_norm, "!=", A.ZERO):
                nvel = A.vdiv(rel_vel, vel_norm)
                cur = current_vector(A, htype, p, rel_vel, a.goal, obstacles, i, a.rot)
                k = A.div(A.c(k_circ) if not isinstance(k_circ, Q) else k_circ, A.mul(dist, dist))
                terms.append(A.vscale(k, A.cross(nvel, A.cross(cur, nvel))))
    return terms


def repel_force(A, a, obstacles, k_repel):
    """CfAgent::repelForce (B/src/cf_agent.cpp:159-181): the last obstacle only"""
    o = obstacles[-1]
    p = a.latest
    dist = _floored_dist(A, p, o, a.rad)
    if A.decide("shell", dist, "<", a.shell):
        u = A.normalized(A.vsub(p, o.pos))
        t = A.sub(A.div(A.ONE, dist), A.div(A.ONE, a.shell))
        dd = A.mul(dist, dist)
        return A.vdiv(A.vscale(t, A.vscale(A.c(k_repel), u)), dd)
    return None


def attractor_force(A, a, k_attr, k_damp, k_goal_scale):
    """CfAgent::attractorForce (B/src/cf_agent.cpp:183-193)"""
    if k_attr == 0.0:
        return None
    goal_vec = A.vsub(a.goal, a.latest)
    vel_des = A.vscale(A.div(A.c(k_attr), A.c(k_damp)), goal_vec)
    n = A.norm(vel_des)
    if n.v == 0 and n.e == 0:
        lim = A.ONE                                 # vel_max / 0 = inf; min(1, inf) = 1
    else:
        lim = A.smin("scale_lim", A.ONE, A.div(a.vel_max, n))
    vel_des = A.vscale(lim, vel_des)
    return A.vscale(A.mul(k_goal_scale, A.c(k_damp)), A.vsub(vel_des, a.vel))


def attractor_force_scaling(A, a, obstacles):
    """CfAgent::attractorForceScaling (B/src/cf_agent.cpp:195-227)"""
    p = a.latest
    closest = a.shell
    cid = None
    for i in range(len(obstacles) - 1):
        d = _floored_dist(A, p, obstacles[i], a.rad)
        if A.decide("scale_closest", d, "<", closest):
            closest, cid = d, i
    A.note("scale_none", cid is None)
    if cid is None:
        return A.ONE
    goal_vec = A.vsub(a.goal, p)
    if (A.decide("scale_zero", A.dot(goal_vec, a.vel), "<=", A.ZERO)
            and A.decide("scale_zero", A.norm(a.vel), "<", A.sub(a.vel_max, A.mul(A.c(0.1), a.vel_max)))
            and A.decide("scale_zero", A.norm(goal_vec), ">", A.c(0.15))):
        return A.ZERO
    w1 = A.sub(A.ONE, A.exp(A.div(A.neg(A.sqrt(closest)), a.shell)))
    ro = A.vsub(obstacles[cid].pos, p)
    w2 = A.sub(A.ONE, A.div(A.dot(goal_vec, ro), A.mul(A.norm(goal_vec), A.norm(ro))))
    w2 = A.mul(w2, w2)
    return A.mul(w1, w2)


def update_position_and_velocity(A, a, force, dt):
    """CfAgent::updatePositionAndVelocity (B/src/cf_agent.cpp:253-268)"""
    dt = A.c(dt)
    acc = A.vdiv(force, a.mass)
    acc_norm = A.norm(acc)
    if A.decide("acc_clamp", acc_norm, ">", A.c(13.0)):
        acc = A.vscale(A.div(A.c(13.0), acc_norm), acc)
    half = A.vscale(dt, A.vscale(dt, A.vscale(A.c(0.5), acc)))
    vdt = A.vscale(dt, a.vel)
    p = a.latest
    new_pos = tuple(A.sum_any([p[k], half[k], vdt[k]]) for k in range(3))
    vel = A.vadd(a.vel, A.vscale(dt, acc))
    vn = A.norm(vel)
    if A.decide("vel_clamp", vn, ">", a.vel_max):
        vel = A.vscale(A.div(a.vel_max, vn), vel)
    a.vel = vel
    a.acc = acc
    a.path.append(new_pos)


def gate_open(A, a):
    """!(getDistFromGoal() < approach_dist_ || (vel_.norm() < 0.5 vel_max_ && (p - init_pos_).norm() < 0.2))
    (B/src/cf_agent.cpp:315-317, 287-289, 352-354)"""
    if A.decide("gate", dist_from_goal(A, a), "<", a.approach):
        return False
    if A.decide("gate", A.norm(a.vel), "<", A.mul(A.c(0.5), a.vel_max)):
        if A.decide("gate", A.norm(A.vsub(a.latest, a.init_pos)), "<", A.c(0.2)):
            return False
    return True


def step(A, a, obstacles, gains, dt, track_min=True, htype=None, hrand=None):
    """one body of the cfPrediction / cfPlanner loop without the obstacle advance (B/src/cf_agent.cpp:313-326,
    285-298, 350-364). gains = (k_attr, k_circ, k_repel, k_damp)"""
    k_attr, k_circ, k_repel, k_damp = gains
    htype = a.type if htype is None else htype
    hrand = a.rand if hrand is None else hrand
    k_goal_scale = A.ONE
    circ = []
    if gate_open(A, a):
        circ = circ_terms(A, a, obstacles, k_circ, track_min, htype, hrand)
        f = A.vsum_any(circ)
        if A.decide("force_gate", A.norm(f), ">", A.c(1e-5)):
            k_goal_scale = attractor_force_scaling(A, a, obstacles)
    rep = repel_force(A, a, obstacles, k_repel)
    att = attractor_force(A, a, k_attr, k_damp, k_goal_scale)
    force = A.vsum_any(circ + [t for t in (rep, att) if t is not None])
    a.force = force
    update_position_and_velocity(A, a, force, dt)


def predict_obstacles(A, obstacles, dt):
    """CfAgent::predictObstacles (B/src/cf_agent.cpp:270-276)"""
    dt = A.c(dt)
    for o in obstacles:
        o.pos = A.vadd(o.pos, A.vscale(dt, o.vel))


def prediction(A, a, obstacles, gains, dt, cap):
    """the cfPrediction inner loop to its guard, and reached_goal_ (B/src/cf_agent.cpp:310-337); obstacles is the agent's
    private copy and advances"""
    ran = False
    while A.decide("guard", dist_from_goal(A, a), ">", A.c(0.1)) and len(a.path) < cap:
        ran = True
        step(A, a, obstacles, gains, dt)
        predict_obstacles(A, obstacles, dt)
    if ran:
        a.reached_goal = A.decide("reached", dist_from_goal(A, a), "<", A.c(0.100001))
    return ran


def set_velocity(A, a, vel):
    """CfAgent::setVelocity (B/src/cf_agent.cpp:54-61)"""
    v = A.v3(vel)
    n = A.norm(v)
    if A.decide("setvel_clamp", n, ">", a.vel_max):
        v = A.vscale(A.div(a.vel_max, n), v)
    a.vel = v


# ---------------------------------------------------------------------------------------------------------------------
# manager: B/src/cf_manager.cpp
# ---------------------------------------------------------------------------------------------------------------------
def path_length(A, path):
    """CfAgent::getPathLength (B/src/cf_agent.cpp:26-32): sequential sum of segment norms"""
    total = A.ZERO
    for i in range(len(path) - 1):
        total = A.add(total, A.norm(A.vsub(path[i + 1], path[i])))
    return total


def agent_cost(A, path, min_obs_dist, goal, approach, cost_gains, ws):
    """one agent's cost in CfManager::evaluateAgents (B/src/cf_manager.cpp:298-334). path: exact points"""
    k_goal, k_len, k_safe, k_ws = [A.c(g) for g in cost_gains]
    pts = [A.v3(q) for q in path]
    cost = A.ZERO
    for q in pts:
        for k in range(3):
            hi, lo = A.c(ws[2 * k]), A.c(ws[2 * k + 1])
            lim = None
            if A.decide("ws", q[k], ">", hi):
                lim = hi
            elif A.decide("ws", q[k], "<", lo):
                lim = lo
            if lim is not None:
                t = A.mul(A.sub(q[k], lim), k_ws)        # |x - lim| * k: the sign is dropped by the square
                cost = A.add(cost, A.mul(t, t))
    g = A.norm(A.vsub(A.v3(goal), pts[-1]))
    if A.decide("goal_cost", g, ">", A.c(approach)):
        cost = A.add(cost, A.mul(g, k_goal))
    cost = A.add(cost, A.mul(path_length(A, pts), k_len))
    mod = A.c(min_obs_dist)
    cost = A.add(cost, A.div(k_safe, mod))
    if A.decide("penalty", mod, "<", A.c(2e-5)):
        cost = A.add(cost, A.c(10000.0))
    return cost


def select_best(A, costs, prev_best_id, keys=None):
    """argmin (first minimum, from numeric_limits::max) and the 0.9 hysteresis (B/src/cf_manager.cpp:335-355).
    prev_best_id: 1-based id of best_agent_, 0 if none. keys: per agent, a value identifying the inputs of its cost (its
    path and min_obs_dist); agents with equal keys have bit-identical fp64 costs, an exact tie. Returns the 0-based
    index evaluateAgents returns.
    The sequential `costs[idx] < min_cost` scan returns the first index of the smallest cost; that is decided when the
    smallest cost is decidedly below every other, or exactly tied with later agents of the same key -- comparisons
    between two costs that are both above the minimum do not change the result."""
    idx = min(range(len(costs)), key=lambda i: (costs[i].v, i))
    for j, c in enumerate(costs):
        if j == idx:
            A.note("argmin", True)                    # below the running minimum when the scan reaches it
        elif keys is not None and keys[j] == keys[idx]:
            if j < idx:
                raise Undecidable("argmin")           # (cannot happen: equal keys, equal values, the lower index wins)
            A.note("argmin", False)                   # equal bits: not <
        elif not A.decide("argmin", c, ">", costs[idx]):
            raise Undecidable("argmin")
        else:
            A.seen["argmin"].add(False)
    if prev_best_id:
        if A.decide("hysteresis", costs[idx], "<", A.mul(A.c(0.9), costs[prev_best_id - 1])):
            return idx
        return prev_best_id - 1
    return idx


def body_force(A, link_pos, k_r_force, obstacles, *, shell, rad):
    """CfManager::getLinkForce -> CfAgent::bodyForce (B/src/cf_manager.cpp:169-182, B/src/cf_agent.cpp:229-234)"""
    a = Agent(A, link_pos, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), [], [], shell=shell, mass=1.0,
              rad=rad, vel_max=1.0, approach=0.0, atype=REAL)
    r = repel_force(A, a, obstacles, k_r_force)
    return r if r is not None else A.v3((0.0, 0.0, 0.0))


def eval_obstacle_distance(A, pos, obstacles, *, shell, rad):
    """CfAgent::evalObstacleDistance (B/src/cf_agent.cpp:146-157): every obstacle, the sentinel included, no floor"""
    p = A.v3(pos)
    best = A.c(shell)
    r = A.c(rad)
    for o in obstacles:
        d = A.sub(A.norm(A.vsub(p, o.pos)), A.add(r, o.rad))
        if A.decide("eod_min", best, ">", d):
            best = d
    return best


# ---------------------------------------------------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------------------------------------------------
def excess(q, x):
    """|x - q.v| / q.e for an fp64 result x (0 if equal, inf if q is exact and x differs)"""
    d = abs(MPF(float(x)) - q.v)
    if d == 0:
        return 0.0
    if q.e == 0.0:
        return math.inf
    return float(d) / q.e
