/*
 * pmaf.h -- C-ABI of the MI355X-native predictive multi-agent circular-field
 * planner tick (libpmaf_hip.so, hand-written HIP kernels for gfx950).
 *
 * This is the drop-in boundary for ONE path of the reference
 * (riddhiman13/predictive-multi-agent-framework, package bimanual_planning_ros):
 * the per-tick forward rollout of N virtual agents over an H-step horizon,
 * scoring, best-agent selection and the real agent's single step. The
 * reference has no FFI for it -- ghostplanner::cfplanner::CfManager is a plain
 * C++ class compiled into the planner node -- so every entry point below cites
 * the CfManager / CfAgent member it replaces (B/ = src/bimanual_planning_ros/).
 * The C++ facade in include/bimanual_planning_ros/cf_manager.h re-creates the
 * reference's class surface on top of these calls.
 *
 * Conventions
 *  - all arithmetic is IEEE double; flat row-major arrays; plain pointers.
 *    Every operation of the default kernels is the correctly rounded one the
 *    reference's compiled code performs, in its order (pmaf_eval_order); exp()
 *    (B/src/cf_agent.cpp:220) is glibc >= 2.28's algorithm restated
 *    (csrc/pmaf_device.hpp: portable_exp): the bits of std::exp on x86-64
 *    glibc hosts with FMA.
 *  - a handle batches P independent populations ("scenes": one CfManager
 *    each); every array argument carries a leading [P] dimension. The
 *    reference's single-manager use is P = 1.
 *  - obstacles are [P][n_obstacles][7] = px,py,pz,vx,vy,vz,radius. The LAST
 *    obstacle of a population is the repulsive-only one
 *    (B/src/cf_agent.cpp:159-181, reference README.md:80); the others generate
 *    circular fields (B/src/cf_agent.cpp:75).
 *  - agent index is 0-based (as returned by CfManager::evaluateAgents), agent
 *    IDs inside the handle are 1-based like the reference.
 *  - every function returns PMAF_OK (0) or a negative pmaf_status; the message
 *    is available from pmaf_last_error(). Nothing throws across the ABI.
 *  - a handle is not thread-safe (neither is CfManager: all calls come from the
 *    single-threaded ROS spinner, B/src/panda_bimanual_control.cpp:475).
 *  - numeric range: every input value must be finite and either 0 or
 *    2^-100 <= |x| <= 2^100 (PMAF_ERR_INVALID otherwise).
 *  - there is NO CPU fallback: without a HIP device pmaf_create fails with
 *    PMAF_ERR_DEVICE.
 */
#ifndef PMAF_H
#define PMAF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMAF_ABI_VERSION 7   /* 7: pmaf_pick_lanes_per_agent / pmaf_estimate_rollout_us (the mapping rule as a pure function), pmaf_get_priority_slices;
                              * pmaf_move_real with steps = 0 leaves no trace; 6: pmaf_eval_order (build-time evaluation-order policy); pmaf_set_real_position no longer waits
                              * for the running rollout; 5: PMAF_FLAG_CONTRACTED, pmaf_get_health, the winner path in pinned
                              * memory, the tick's time limit */

typedef enum pmaf_status {
  PMAF_OK = 0,
  PMAF_ERR_INVALID = -1, /* bad argument (NULL, size <= 0, empty obstacle list ...) */
  PMAF_ERR_DEVICE = -2,  /* HIP runtime / no device */
  PMAF_ERR_STATE = -3,   /* call not valid in the handle's current state */
  PMAF_ERR_NOMEM = -4
} pmaf_status;

/* values of CfAgent::Type, B/include/bimanual_planning_ros/cf_agent.h:59-68 */
typedef enum pmaf_agent_type {
  PMAF_REAL_AGENT = 0,
  PMAF_GOAL_HEURISTIC = 1,
  PMAF_OBSTACLE_HEURISTIC = 2,
  PMAF_GOAL_OBSTACLE_HEURISTIC = 3,
  PMAF_VEL_HEURISTIC = 4,
  PMAF_RANDOM_AGENT = 5,
  PMAF_HAD_HEURISTIC = 6
} pmaf_agent_type;

typedef struct pmaf_planner pmaf_planner;

/* pmaf_params.flags */
/* Opt-in fast arithmetic in the wave-per-agent rollout kernel: divisions and
 * square roots by v_rcp_f64 / v_rsq_f64 + two Newton steps (1-2 ulp) instead of
 * the correctly rounded IEEE sequences. Default (flag clear) is the strict mode
 * whose results are bit-identical to the CPU restatement. */
#define PMAF_FLAG_FAST_MATH 1
/* Use the compiler's fully general IEEE division / sqrt expansions in the
 * rollout kernels instead of the default hand-expanded ones (same bits for
 * all operands within 2^+-250, which the validated input range guarantees;
 * ~13 % slower). See csrc/pmaf_device.hpp "arithmetic policy". */
#define PMAF_FLAG_IEEE_SEQUENCES 2
/* pmaf_tick sleeps (20 us quanta) between its polls of the mailbox's sequence
 * number instead of spinning: no host core is burnt while the previous rollout
 * still runs (batch drivers issuing ticks back to back), at the price of the
 * wake-up latency (set-point up to a quantum + scheduler latency later).
 * Default: spin (lowest set-point latency). */
#define PMAF_FLAG_BLOCKING_WAIT 4
/* Opt-in CONTRACTED arithmetic in the rollout kernels (wave-per-agent and group kernels; ABI 5): PMAF_FLAG_FAST_MATH's
 * reciprocal / reciprocal-square-root sequences AND fused multiply-adds wherever the step forms a * b + c (dot products,
 * cross products, the integrator's a + b * s), plus an unordered (tree) force sum. The step of these kernels is bound
 * by its instruction count, and the FMA is the one FP64 instruction that retires two operations. Results are NOT
 * bit-identical to the CPU restatement. What holds instead (tests/test_tolerance_gpu.py, >= 50 closed-loop ticks against
 * the oracle's libm mode): on WELL-CONDITIONED scenes (BASELINE C1-C4, the six shipped dual_arms_* task scenes) the same
 * best-agent sequence and the selected trajectory within the north star's 1e-5 m; on CHAOTIC scenes it does NOT hold --
 * one of BASELINE C5's eight scenes (3.2e-3 m) and the shipped sim_kobo_dyn_spheres1/2/3 tasks (0.2 m; spheres3 selects
 * another agent at tick 1), the list CONTRACTED_EXCEEDS of that test file. The real agent's step (the set-point that is
 * published) is always evaluated in strict arithmetic. Default: flag clear. */
#define PMAF_FLAG_CONTRACTED 8

/*
 * Arguments of CfManager::init (B/src/cf_manager.cpp:41-124,
 * B/include/bimanual_planning_ros/cf_manager.h:93-102) for P populations.
 */
typedef struct pmaf_params {
  int32_t abi_version;          /* PMAF_ABI_VERSION */
  int32_t n_populations;        /* P >= 1 */
  int32_t n_agents;             /* N = k_a_ee.size() per population */
  int32_t n_obstacles;          /* obstacles.size() = M+1 >= 1 per population */
  int32_t max_prediction_steps; /* path capacity in points (H+1) */
  int32_t device;               /* HIP device ordinal; -1 = current device */
  int32_t lanes_per_agent;      /* 0 = auto; else 1,2,4,8,16,32,64 */
  int32_t flags;                /* PMAF_FLAG_* bits, 0 = defaults */
  double dt;                    /* prediction_freq_multiple * delta_t */
  double velocity_max;
  double approach_dist;
  double detect_shell_rad;
  double agent_mass;            /* reference default 1.0 */
  double radius;                /* reference default 0.05 */
  const double *goal;           /* [P][3] */
  const double *init_pos;       /* [P][3] CfManager::init_pos_ when init runs (agents are built there); NULL = zeros */
  const double *obstacles;      /* [P][n_obstacles][7] */
  const double *k_attr;         /* [P][N] k_a_ee */
  const double *k_circ;         /* [P][N] k_c_ee */
  const double *k_repel;        /* [P][N] k_r_ee */
  const double *k_damp;         /* [P][N] k_d_ee */
  const int32_t *agent_types;   /* [N] or NULL = reference layout Had,Goal,Obstacle,GoalObstacle,Vel,Random... (cf_manager.cpp:70-104) */
  const double *random_vecs;    /* [P][N][n_obstacles][3] unit vectors for Random agents (replaces std::random_device, B/src/helper_functions.cpp:7-13); NULL = all zero */
} pmaf_params;

/* CfManager::init / ~CfManager */
int pmaf_create(const pmaf_params *params, pmaf_planner **out);
int pmaf_destroy(pmaf_planner *h);
const char *pmaf_last_error(void);
int pmaf_abi_version(void);
/* Evaluation-order policy this library was BUILT with (csrc/build.sh, PMAF_VARIANT). The reference's arithmetic is
 * Eigen's, and one detail of it depends on how Eigen was compiled: a fixed-size 3-vector dot product / squaredNorm
 * (every norm, normalisation and projection of B/src/cf_agent.cpp:72-611) sums
 *   (a0 b0 + a1 b1) + a2 b2   PMAF_EVAL_ORDER_DOT_LEFT   Eigen 3.3 with a double-precision packet type: x86-64 SSE2,
 *                             aarch64 NEON (Redux.h, LinearVectorizedTraversal + CompleteUnrolling: predux of the first
 *                             packet, then the remaining coefficient) -- a stock `catkin build`; the DEFAULT library;
 *   a0 b0 + (a1 b1 + a2 b2)   PMAF_EVAL_ORDER_DOT_RIGHT  its non-vectorised redux (redux_novec_unroller splits 3 as
 *                             1 + 2): -DEIGEN_DONT_VECTORIZE, 32-bit ARM ...; the `rassoc` variant library.
 * Both are IEEE-conformant; they differ in the last bit of some sums, and a long rollout through many obstacles can
 * amplify that (profiles/r4_oracle_conditioning.txt: 2.3e-5 m on the shipped dual_arms_static1 scene, decimetres on
 * the sim_kobo_dyn_spheres* tasks). Pick the library whose order matches the Eigen build it replaces; oracle/pin/
 * holds the recipe that tells which one that is. Kernels, the manager's real step and the host-side getters all
 * follow the one switch (-DPMAF_DOT_RIGHT_ASSOC), and so does the CPU oracle the parity suite compares with. */
#define PMAF_EVAL_ORDER_DOT_LEFT 0
#define PMAF_EVAL_ORDER_DOT_RIGHT 1
int pmaf_eval_order(void);

/* CfManager::setInitialPosition, B/src/cf_manager.cpp:226-236. pos [P][3]. Every path restarts at pos. A pmaf_start
 * right behind it launches from the population's reset state (the velocity of the last reset; the creation state before
 * any), not from each agent's own last velocity as the reference's threads would after earlier rollouts: identical on a
 * fresh handle and in front of a tick, whose reset hands every agent the real agent's velocity. */
int pmaf_set_initial_position(pmaf_planner *h, const double *pos);
/* CfManager::setRealEEAgentPosition, B/src/cf_manager.cpp:216-218 -> RealCfAgent::setPosition = push_back
 * (B/src/cf_agent.cpp:44-46): the measured position becomes the real agent's latest one (closed loop: the node calls it
 * in front of every tick when open_loop is false, B/src/panda_bimanual_control.cpp:333-335). pos [P][3]. Returns at once
 * (ABI 6): the position is left in pinned memory and read by the manager kernel of the NEXT pmaf_tick / pmaf_evaluate /
 * pmaf_move_real / pmaf_reset_agents -- no wait for the running rollout, no copy command in front of the tick; the
 * real-agent getters (pmaf_get_real_state, pmaf_get_dist_from_goal, pmaf_get_real_path) show it immediately. */
int pmaf_set_real_position(pmaf_planner *h, const double *pos);

/* CfManager::startPrediction (cf_manager.h:57-61): asynchronous launch of the
 * agent x horizon rollout kernel on the handle's stream. Rollouts always run
 * to their guard (full horizon or goal reached, B/src/cf_agent.cpp:310-311). */
int pmaf_start(pmaf_planner *h);
/* CfManager::stopPrediction (B/src/cf_manager.cpp:126-140): stream sync. */
int pmaf_stop(pmaf_planner *h);

/* The three calls below are what the unchanged node issues per tick (B/src/panda_bimanual_control.cpp:337-351). Each is
 * ONE manager launch whose result the host takes from the mailbox in pinned memory (no stream synchronisation); obstacle
 * lists are handed over through the mapped pinned buffer -- not at all when bit-identical to the resident one -- and
 * agent indices / reset states by value in the kernel arguments for <= 4 populations: the five-call tick costs ~33 us at
 * the C++ boundary, pmaf_tick ~13 us (profiles/r6_facade_latency.txt). */
/* CfManager::evaluateAgents, B/src/cf_manager.cpp:293-356.
 * cost_gains = {k_goal_dist,k_path_len,k_safe_dist,k_workspace},
 * ws = {xmax,xmin,ymax,ymin,zmax,zmin}; best_idx [P] out. */
int pmaf_evaluate(pmaf_planner *h, const double *cost_gains, const double *ws,
                  int32_t *best_idx);
/* CfManager::moveRealEEAgent, B/src/cf_manager.cpp:257-263. obstacles
 * [P][n_obstacles][7] live obstacles; agent_id [P]. */
int pmaf_move_real(pmaf_planner *h, const double *obstacles, double dt,
                   int32_t steps, const int32_t *agent_id);
/* CfManager::resetEEAgents, B/src/cf_manager.cpp:246-255. pos, vel [P][3]. */
int pmaf_reset_agents(pmaf_planner *h, const double *pos, const double *vel,
                      const double *obstacles);
/*
 * The planCallback sequence stop -> evaluate -> moveRealEEAgent(1 step) ->
 * resetEEAgents(next pos, next vel) -> start
 * (B/src/panda_bimanual_control.cpp:336-352) as two back-to-back launches.
 * Returns once best_idx / next_pos / next_vel (each [P], [P][3], [P][3]; may be
 * NULL) are on the host; the new rollout keeps running asynchronously, like
 * the reference's prediction threads. obstacles may be NULL (= unchanged).
 * A list that differs from the previous one in a field obstacle (compared bit for
 * bit) and is at rest makes the next reset recompute the Obstacle / GoalObstacle
 * heuristics' closest-other table (populations of more than 60 field obstacles on
 * the wave-per-agent kernels; M distances per obstacle, once): passing the same
 * static list every tick, as the reference's node does, costs nothing.
 */
int pmaf_tick(pmaf_planner *h, const double *obstacles, double dt,
              const double *cost_gains, const double *ws, int32_t *best_idx,
              double *next_pos, double *next_vel);

/* ---- failure detection on the tick (ABI 5; SURVEY.md section 5: the reference has none for the planner -- its consumer
 * logs a NaN set-point, B/src/costp_controller.cpp:317-319) ----
 * Time limit: pmaf_tick waits for the manager kernel's result at most PMAF_TICK_TIMEOUT_S seconds (environment, read
 * at pmaf_create; default 5) and then fails with PMAF_ERR_DEVICE instead of spinning on a hung device; the outputs are
 * not written in that case. The two kernels of that tick are still queued or running then (they read the call's staging
 * buffers and write the mailbox later), so the handle refuses every further pmaf_tick with PMAF_ERR_STATE until
 * pmaf_stop() has drained the stream (or the handle is recreated). A failed pmaf_tick never counts its obstacle list as
 * handed over: the retry passes it again.
 * Health word of the last pmaf_tick / pmaf_evaluate / pmaf_move_real per population (bits below), written by the
 * manager kernel next to the set-point. pmaf_tick itself still returns PMAF_OK with the (NaN) set-point in its
 * outputs -- the reference's planner publishes it too -- the caller decides (the C++ facade's planTick throws). */
#define PMAF_HEALTH_SETPOINT_NAN 1   /* the real agent's next position / velocity is not finite */
#define PMAF_HEALTH_FORCE_NAN 2      /* the force on the real agent is not finite (e.g. the Had heuristic's rotation vector
                                        for an obstacle centre on the agent-goal line, B/src/cf_agent.cpp:599-611) */
#define PMAF_HEALTH_ACC_CLAMPED 4    /* updatePositionAndVelocity's |a| <= 13 clamp acted on the real agent's step */
#define PMAF_HEALTH_COST_NAN 8       /* no agent had a comparable cost (all NaN): index 0 was kept, as the reference does */
int pmaf_get_health(pmaf_planner *h, int32_t *bits /* [P] */);

/* ---- the selected trajectory of every tick on the host (ABI 5) ----
 * What the reference's planCallback hands out per tick (B/src/panda_bimanual_control.cpp:340-347: the predicted paths,
 * the best one marked) without the copy of ALL paths pmaf_view_paths makes: once enabled, the manager kernel of every
 * pmaf_tick / pmaf_evaluate writes the SELECTED agent's path -- as it was scored -- into mapped pinned host memory
 * right behind the set-point (24 B per path point; the rollout launched by the same tick starts behind it).
 * pmaf_view_winner_path waits for the path of the LAST tick / evaluate and returns pointers into that memory:
 * *paths [P][cap][3] (entries past n_points[p] are unspecified), *n_points [P], *agent [P] (0-based index); valid until
 * the next pmaf_tick / pmaf_evaluate. Any of the three may be NULL. */
int pmaf_enable_winner_path(pmaf_planner *h, int32_t enable);
int pmaf_view_winner_path(pmaf_planner *h, const double **paths, const int32_t **n_points, const int32_t **agent);
/* entry of pmaf_tick -> the winner path on the host (pmaf_view_winner_path's return), library clock, microseconds;
 * one sample per pmaf_view_winner_path call that followed a pmaf_tick, oldest first; clears the record */
int pmaf_get_winner_path_times_us(pmaf_planner *h, double *out, int32_t max_n, int32_t *n);

/* ---- synchronous stepping API of the class surface (no callers in the reference) ----
 * CfManager::moveAgents / moveAgentsPar (B/src/cf_manager.cpp:274-291) ->
 * CfAgent::cfPlanner (B/src/cf_agent.cpp:278-300): every agent takes `steps`
 * steps of length dt from its CURRENT state through the caller's obstacle list
 * [P][n_obstacles][7] (positions, velocities and radii as given; no obstacle
 * advance, no loop guard). Paths are bounded by max_prediction_steps here
 * (PMAF_ERR_STATE if a path would outgrow it; the reference's grow without
 * bound). After a stepping call pmaf_start needs a pmaf_reset_agents /
 * pmaf_set_* first (rollouts start from the population's reset state). */
int pmaf_move_agents(pmaf_planner *h, const double *obstacles, double dt, int32_t steps);
/* CfManager::moveAgent (B/src/cf_manager.cpp:265-272): agent agent_id[p] repeats
 * cfPlanner(steps) while it is farther than 0.05 from the goal -- at most
 * max_calls times and while the path buffer has room; calls [P] (may be NULL)
 * = cfPlanner calls made. */
int pmaf_move_agent(pmaf_planner *h, const double *obstacles, double dt, int32_t steps,
                    const int32_t *agent_id, int32_t max_calls, int32_t *calls);
/* CfManager::setEEAgentPositions (B/src/cf_manager.cpp:220-224): every agent's
 * path restarts at pos [P][3]; velocities stay (for the stepping calls that
 * follow). Deviation: like after pmaf_move_agent(s), pmaf_start then needs a
 * pmaf_reset_agents / pmaf_set_initial_position first (PMAF_ERR_STATE
 * otherwise) -- in the reference a startPrediction() here would continue with
 * each agent's OWN velocity, known flags and advanced obstacle copies
 * (CfAgent::setPosition only clears the path, B/src/cf_agent.cpp:39-42), which
 * a rollout launched from the population's reset state cannot reproduce. The
 * reference has no caller of this method. */
int pmaf_set_agent_positions(pmaf_planner *h, const double *pos);
/* CfManager::setEEAgentPosAndVels (B/src/cf_manager.cpp:238-244): pos, vel [P][3]
 * (velocity clamped to velocity_max, CfAgent::setVelocity). Same rule for a
 * following pmaf_start as pmaf_set_agent_positions. */
int pmaf_set_agent_pos_and_vels(pmaf_planner *h, const double *pos, const double *vel);
/* CfAgent::evalObstacleDistance (B/src/cf_agent.cpp:146-157) of every agent at
 * its latest position against obstacles [P][n_obstacles][7]; out [P][N]. */
int pmaf_eval_obstacle_distance(pmaf_planner *h, const double *obstacles, double *out);

/* ---- path audit: the predicted paths against a LIVE obstacle list (exports added under ABI 7) ----
 * The reference declares `double CfManager::evaluatePath(const std::vector<Obstacle> &obstacles)`
 * (B/include/bimanual_planning_ros/cf_manager.h:130) and never defines it. CfManager::evaluateAgents takes the tick's
 * fresh obstacle list and IGNORES it (B/src/cf_manager.cpp:293-356): its safety term is min_obs_dist_, recorded by the
 * rollout against the obstacle copies of the previous reset -- field obstacles only, ungated steps only, floored at
 * 1e-5 and capped at the shell radius (B/src/cf_agent.cpp:83-88). These two calls answer what that leaves open once the
 * obstacles have moved: how close does each candidate path come to the list as it is NOW, to which obstacle, at which
 * step, and from which step on is it no longer clear.
 * For population p, agent a, the handle's CURRENT predicted paths x_0 .. x_{n-1} (n = n_points[p][a]; whatever wrote
 * them: a rollout or the stepping calls) and EVERY obstacle j of obstacles [P][n_obstacles][7], the trailing repulsive
 * one included:
 *   o_j^0 = the given position, o_j^{k+1} = o_j^k + v_j * dt  per component, one multiply then one add, each rounded
 *           (iterated like CfAgent::predictObstacles, B/src/cf_agent.cpp:270-276; dt = pmaf_params.dt)
 *   c(k,j) = norm(x_k - o_j^k) - (radius + r_j)               (evalObstacleDistance, B/src/cf_agent.cpp:150-151;
 *           norm = sqrt(dot) in the build's association, pmaf_eval_order; no floor, no cap: negative = penetration)
 * clearance [P][N]       = min over (k,j) of c, found with a strict `<` from +infinity (a NaN pair never wins);
 * step, obstacle [P][N]  = its argmin; ties go to the smallest k, then the smallest j; -1 when no pair won;
 * first_violation [P][N] = the smallest k with c(k,j) < margin for some j, else n;
 * per_obstacle [P][N][n_obstacles] = min over k of c(k,j).
 * step / obstacle / first_violation / per_obstacle may each be NULL. An empty path gives +infinity, -1, -1, 0.
 * Like the getters of rollout results the calls wait for the running rollout; they change no planner state (a tick
 * sequence with audits in between is bit-identical to one without). The reference left the return value of
 * evaluatePath open; here it is the clearance in metres. */
int pmaf_evaluate_paths(pmaf_planner *h, const double *obstacles, double margin, double *clearance, int32_t *step,
                        int32_t *obstacle, int32_t *first_violation, double *per_obstacle);
/* CfManager::evaluatePath (declared at B/include/bimanual_planning_ros/cf_manager.h:130, undefined in the reference;
 * evaluateAgents ignores its list, B/src/cf_manager.cpp:293-356): the clearance, as above, of the SELECTED agent's
 * current path only; clearance [P]. PMAF_ERR_STATE before the first selection (pmaf_evaluate / pmaf_tick). */
int pmaf_evaluate_path(pmaf_planner *h, const double *obstacles, double *clearance);

/* ---- cross audit: two sets of predicted paths against each other; the pair pick (exports added under ABI 7) ----
 * A bimanual planner runs one population per arm. What one arm's rollouts see of the other is a single sphere at the
 * other arm's last published set-point (the trailing repulsive obstacle); pmaf_evaluate scores each population alone,
 * and pmaf_evaluate_paths holds paths against spheres on straight constant-velocity tracks, which the other arm's
 * predicted path is not. These calls hold the two arms' candidate paths against each other, step by step (SURVEY.md
 * 8(e): the other arm's "winning path, sampled at the same step"). No reference equivalent.
 * Two path sets of one handle share dt and max_prediction_steps (cap). Path i of set A has the points x_0 .. x_{n-1},
 * path j of set B the points y_0 .. y_{m-1}; both rollouts start at the same tick, so step k of both is one instant.
 *   hold:       a path that has ended (goal guard, the stepping calls) stays at its last point:
 *               xh_k = x_{min(k, n-1)}, yh_k = y_{min(k, m-1)}, for k < K = max(n, m)
 *   empty:      n == 0 or m == 0: clearance +infinity, step -1
 *   d2(k)     = dot(xh_k - yh_k, xh_k - yh_k) in the build's dot association (pmaf_eval_order), every operation
 *               rounded, nothing fused
 *   step(i,j) = argmin over k of d2(k), found with a strict `<` from +infinity, k ascending: ties go to the smallest
 *               k, a NaN never wins; -1 if none won
 *   clearance(i,j) = sqrt(d2(step)) - separation, +infinity if none won. separation = the caller's sum of the two
 *               bodies' radii (for shard.DualArmCoupling: pmaf_params.radius + its self-collision radius); no floor,
 *               no cap, negative = penetration.
 * The minimum is defined on d2, not on its root: sqrt is correctly rounded and therefore monotone, so clearance equals
 * the minimum over k of sqrt(d2(k)) - separation bit for bit; only the tie rule of `step` depends on the choice.
 * All three calls wait for the running rollout like the getters of its results and change no planner state (a tick
 * sequence with these calls in between is bit-identical to one without).
 *
 * pmaf_cross_audit: set A = population pop_a's CURRENT paths, set B = population pop_b's, read where they lie on the
 * device. clearance [N][N] (row i = agent i of pop_a), step [N][N] or NULL. PMAF_ERR_INVALID for pop_a == pop_b or an
 * index outside [0, P). */
int pmaf_cross_audit(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, double *clearance, int32_t *step);
/* Set B from the caller: the other arm when it lives in another handle or on another GPU (its selected path is on
 * every rank in the winner records; through the facade, the paths of a second CfManager). tracks
 * [n_tracks][cap][3] with cap = max_prediction_steps, n_track_points [n_tracks]; rows past a track's count are not
 * read, the others are range-checked like every input. clearance [N][n_tracks], step likewise or NULL.
 * PMAF_ERR_INVALID for n_tracks <= 0 or a count outside [0, cap]. */
int pmaf_cross_audit_tracks(pmaf_planner *h, int32_t pop, int32_t n_tracks, const double *tracks,
                            const int32_t *n_track_points, double separation, double *clearance, int32_t *step);
/* The cheapest pair of candidates that keeps its distance. cost_a[i], cost_b[j] = what pmaf_get_costs returns at this
 * moment for the two populations (read from the same device array behind the same wait: whatever that getter reports
 * in a state of the handle -- zeros before the first pmaf_evaluate / pmaf_tick made cost parameters known -- is what
 * this call uses, and it fails where and how that getter fails).
 *   feasible(i,j) iff clearance(i,j) >= margin                 (false for NaN, true for +infinity)
 *   among feasible pairs: the minimum of S = cost_a[i] + cost_b[j] (one rounded add), strict `<` from +infinity in
 *   row-major order: ties go to the smallest i, then the smallest j; a NaN sum never wins. -> *feasible = 1
 *   if no pair won: *feasible = 0 and the pair of the greatest clearance, strict `>` from -infinity in row-major order;
 *   if still none won: pair = (-1, -1).
 * pair [2] = (i, j); *pair_cost = S and *pair_clearance = clearance of the returned pair, both NaN for (-1, -1). The
 * matrix stays on the device between the audit and the reduction; only these results come back. The call selects
 * NOTHING in the handle: the caller applies the pair through what exists -- pmaf_move_real's agent_id (or
 * pmaf_set_best). pmaf_move_real's agent_id selects the GAINS of the real step only: its heuristic type and Random
 * vectors are those of the best-agent copy the last pmaf_evaluate made. pmaf_adopt_best (below) makes that copy -- and
 * with it the heuristic -- follow the pair. Intended five-call tick of a bimanual node, both arms in one handle:
 *   pmaf_stop -> pmaf_evaluate -> pmaf_select_pair -> pmaf_move_real(agent_id = pair) -> pmaf_reset_agents -> pmaf_start
 * Right after pmaf_tick the call is pointless: that call has already moved, reset and restarted, so the paths in the
 * handle belong to the NEW rollout while the costs still describe the old one. Hysteresis over pairs is the caller's
 * (it has both costs and can apply evaluateAgents' 0.9 rule). */
int pmaf_select_pair(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, double margin, int32_t *pair,
                     double *pair_cost, double *pair_clearance, int32_t *feasible);

/* ---- cross audit with timing slack: arms that run late still keep apart (exports added under ABI 7) ----
 * The cross audit above rests on "step k of both is one instant". On a robot that does not hold: the real end-effector
 * trails its set-points (the closed-loop scenarios put a 30 % tracking lag in the loop), and the two arms' controllers
 * do not trail by the same amount. A pair that is clear step against step can collide when one arm is three steps
 * behind its schedule. These calls audit the same two path sets over a WINDOW of relative delays.
 * Everything the block above defines carries over unchanged: path i of set A has the points x_0 .. x_{n-1}, path j of
 * set B the points y_0 .. y_{m-1}; the hold rule xh_k = x_{min(k, n-1)}, yh_l = y_{min(l, m-1)} with K = max(n, m);
 * dot in the build's association (pmaf_eval_order), every operation rounded, nothing fused.
 * The slack is two non-negative step counts:
 *   late_a:     A may be up to late_a steps behind B's clock: A stands at xh_k while B is already at yh_{k+s},
 *               0 <= s <= late_a
 *   late_b:     the same the other way round
 *   admitted:   an index pair (k, l), 0 <= k, l < K, iff -late_b <= l - k <= late_a. Because of the hold rule this
 *               window over [0, K)^2 covers every instant of every delay in range: a late arm waits at its point 0
 *               before it starts, an ended arm waits at its last point.
 *   d2(k, l)  = dot(xh_k - yh_l, xh_k - yh_l)
 *   (step_a, step_b)(i,j) = the admitted pair that is smallest under the total order (d2, k, l): what a scan with k
 *               ascending, then l ascending, and a strict `<` from +infinity finds. A NaN never wins; (-1, -1) when
 *               nothing won.
 *   clearance(i,j) = sqrt(d2(step_a, step_b)) - separation; +infinity when nothing won or a path is empty (n == 0 or
 *               m == 0). No floor, no cap.
 *   late_a < 0 or late_b < 0: PMAF_ERR_INVALID. Values >= max_prediction_steps mean every pair of steps (they are
 *               clamped on the host before any device arithmetic: no index computation can overflow).
 * Consequences:
 *   - with (late_a, late_b) = (0, 0) the results equal pmaf_cross_audit's bit for bit, and step_a = step_b = step
 *     (the calls below still run their own kernel then);
 *   - the clearance never grows when either slack grows (the admitted set only gains pairs);
 *   - audit(A, B, late_a, late_b) has the transposed clearance bits of audit(B, A, late_b, late_a): the admitted sets
 *     are mirror images and d2 is symmetric bit for bit. The STEPS transpose only where the minimum is unique: the tie
 *     rule is lexicographic in (k, l), A's step first, and the mirror image of its winner need not be the winner of
 *     the mirrored scan (a minimum reached at (2, 5) and at (3, 4) is reported as (2, 5); the mirrored call sees it at
 *     (5, 2) and (4, 3) and reports (4, 3), the mirror image of (3, 4)).
 * Waiting, state and validation are those of the three calls above: the calls wait for the running rollout, change no
 * planner state, and range-check population indices, track counts and inputs the same way.
 *
 * pmaf_cross_audit_slack: clearance [N][N], step_a / step_b [N][N], each NULL or given. */
int pmaf_cross_audit_slack(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, int32_t late_a, int32_t late_b,
                           double *clearance, int32_t *step_a, int32_t *step_b);
/* Set B from the caller, as pmaf_cross_audit_tracks: clearance [N][n_tracks], step_a / step_b likewise or NULL. */
int pmaf_cross_audit_tracks_slack(pmaf_planner *h, int32_t pop, int32_t n_tracks, const double *tracks,
                                  const int32_t *n_track_points, double separation, int32_t late_a, int32_t late_b,
                                  double *clearance, int32_t *step_a, int32_t *step_b);
/* pmaf_select_pair's rule, exactly, on the slacked matrix (which stays on the device): feasible iff clearance >= margin,
 * then the minimum of cost_a[i] + cost_b[j], else the greatest clearance, ties in row-major order. pair_steps [2] or
 * NULL: (step_a, step_b) of the returned pair's matrix entry, (-1, -1) for the pair (-1, -1). The five-call tick:
 *   pmaf_stop -> pmaf_evaluate -> pmaf_select_pair_slack -> pmaf_move_real(agent_id = pair) -> pmaf_reset_agents -> pmaf_start */
int pmaf_select_pair_slack(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, double margin, int32_t late_a,
                           int32_t late_b, int32_t *pair, double *pair_cost, double *pair_clearance, int32_t *feasible,
                           int32_t *pair_steps);

/* ---- selection against the live list; adopting a pick (exports added under ABI 7) ----
 * pmaf_evaluate restates CfManager::evaluateAgents (B/src/cf_manager.cpp:293-356): its safety term is min_obs_dist,
 * recorded against the obstacle copies of the previous reset, and it ignores the list it is given. The audits above
 * say which paths the list as it is NOW blocks, but select nothing. pmaf_select_clear selects: the cheapest agent whose
 * path is clear of the live list, on the device. No reference equivalent.
 * The audit window. For population p and agent a with n = n_points[p][a], the window is the first w = min(n, horizon)
 * points of the CURRENT path. horizon < 1: PMAF_ERR_INVALID; values above max_prediction_steps mean the whole path
 * (clamped on the host). Inside the window everything is pmaf_evaluate_paths' contract, unchanged: the obstacle track is
 * iterated, one multiply then one add per component, each rounded; c(k,j) = norm(x_k - o_j^k) - (radius + r_j) in the
 * build's dot association; every obstacle of obstacles [P][n_obstacles][7] counts, the trailing one included; the
 * minimum is found with a strict `<` from +infinity; a NaN pair never wins and never violates. Per agent:
 *   c_a      = min over k < w and j of c(k,j); +infinity for w = 0
 *   fv_a     = the smallest k < w with c(k,j) < margin for some j, else w
 *   clear_a  iff fv_a == w
 * bit for bit what pmaf_evaluate_paths gives on the paths cut to w points.
 * The rule. cost[a] = what pmaf_get_costs reports at this moment (read from the same device array behind the same
 * wait, as pmaf_select_pair does).
 *   m        = the clear agent of minimum cost: strict `<` from +infinity over ascending index (ties go to the
 *              smallest index; a NaN or +infinite cost never wins)
 *   rule 0   (keep the previous pick) when m exists, prev_idx is given, q = prev_idx[p] >= 0, clear_q holds and
 *              cost[m] >= 0.9 * cost[q]: pick = q. evaluateAgents' hysteresis (:344-350) on the clear set, with one
 *              deliberate difference: a previous pick whose cost is NaN is NOT kept (the reference's !(a < b) keeps it)
 *   rule 1   (cheapest clear) when m exists and rule 0 does not apply: pick = m
 *   rule 2   (fallback) when m does not exist -- no clear agent, or none with a comparable cost: the agent that stays
 *              clear longest: greatest fv_a, then greatest c_a, then smallest index (a strict scan over ascending
 *              index: the pick is always in [0, N))
 * pick [P] is required; rule [P], n_clear [P] (number of clear agents), cost [P], clearance [P], first_violation [P]
 * (cost, c and fv of the pick) may each be NULL. prev_idx [P] or NULL; an entry outside [-1, N) is PMAF_ERR_INVALID;
 * margin and the list are range-checked like every input.
 * State. With adopt == 0 the call changes no planner state (the list does NOT become the resident live list either: a
 * tick sequence with such calls in between is bit-identical to one without). With adopt != 0 every population adopts
 * its pick exactly as pmaf_adopt_best does. The call waits for the running rollout like the getters do and refuses a
 * handle whose tick was abandoned (PMAF_ERR_STATE until pmaf_stop). Right after pmaf_tick the call is pointless, for
 * the reason given at pmaf_select_pair. Intended six-call tick:
 *   pmaf_stop -> pmaf_evaluate -> pmaf_select_clear(adopt = 1) -> pmaf_move_real(agent_id = pick) -> pmaf_reset_agents -> pmaf_start */
int pmaf_select_clear(pmaf_planner *h, const double *obstacles, double margin, int32_t horizon, const int32_t *prev_idx,
                      int32_t adopt, int32_t *pick, int32_t *rule, int32_t *n_clear, double *cost, double *clearance,
                      int32_t *first_violation);
/* The device-side best_agent_ = ee_agents_[i]->makeCopy() (B/src/cf_manager.cpp:346) for i = agent_idx[p]; agent_idx
 * [P], an entry of -1 leaves that population alone, any other entry outside [0, N) is PMAF_ERR_INVALID. The stores are
 * those of the selection inside pmaf_evaluate when it takes a new agent: has_best = 1, best id = i + 1, best type =
 * the agent's type, best index = i, and the best agent's Random vectors <- agent i's. Enqueued on the handle's stream;
 * no host copy of the vectors is made. Afterwards pmaf_get_best and pmaf_evaluate_path speak of the adopted agent, the
 * next pmaf_move_real steps with its heuristic and vectors, and the next pmaf_evaluate applies its hysteresis to it. The
 * real agent's own rotation vectors and known flags stay, as they do across a selection. Winner records and the winner
 * path keep describing pmaf_evaluate's selection. */
int pmaf_adopt_best(pmaf_planner *h, const int32_t *agent_idx);

/* ---- joint selection: clear of the live list and of each other (exports added under ABI 7) ----
 * pmaf_select_pair picks a pair that keeps apart but may run through an obstacle that has moved since the reset;
 * pmaf_select_clear picks each arm alone, so its two picks may collide with each other. These two calls pick the two
 * arms' agents TOGETHER, on the device: the cheapest pair whose members are both clear of the live list and keep their
 * distance from each other, with hysteresis and a fallback, and -- when asked -- adopt it. No reference equivalent.
 * pmaf_select_pair_clear: side A = population pop_a, side B = population pop_b of the handle.
 * pmaf_select_clear_tracks: side A = population pop, side B = the caller's tracks [n_tracks][cap][3] with
 * n_track_points [n_tracks], as pmaf_cross_audit_tracks takes them (the other arm's selected path when it lives in
 * another handle); track_cost [n_tracks] or NULL.
 * Window. w = min(n_points, horizon) per path, as in pmaf_select_clear; horizon < 1: PMAF_ERR_INVALID; values above
 * max_prediction_steps are clamped on the host. The same window applies to both sides of the cross audit and to the
 * tracks (w = min(n_track_points, horizon)).
 * Obstacle side. Per agent of pop_a and of pop_b, c, fv and clear <=> fv == w are bit for bit pmaf_select_clear's on
 * obstacles [P][n_obstacles][7] and obstacle_margin. With skip_trailing != 0 the obstacle of index n_obstacles - 1 of
 * every list is left out of the audit: in the coupled configuration it is the static sphere at the other arm's last
 * set-point, which the cross audit replaces (the other arm will not stay there). With n_obstacles == 1 that leaves
 * nothing to audit: c = +infinity and every agent is clear. With skip_trailing == 0 every obstacle counts.
 * Pair side. clearance(i,j) and its step(s) are bit for bit what pmaf_cross_audit gives on the two path sets cut to
 * their windows (late == NULL: step against step), or -- late = (late_a, late_b) given -- what pmaf_cross_audit_slack
 * gives on the cut sets, through its own kernel even for (0, 0). A negative entry is PMAF_ERR_INVALID. All windows share
 * one horizon, so the hold rule only ever holds a path that really ended inside the window.
 *   feasible(i,j) iff clear_a[i] and clear_b[j] and clearance(i,j) >= pair_margin   (false for a NaN clearance; tracks:
 *                 clear_b is true for every track)
 *   S(i,j)      = cost_a[i] + cost_b[j], one rounded add; the costs are what pmaf_get_costs reports at this moment, as
 *                 pmaf_select_pair reads them; tracks: cost_b = track_cost, or +0.0 when it is NULL
 *   m           = the feasible pair of least S: strict `<` from +infinity in row-major order (ties go to the smallest
 *                 i, then the smallest j; a NaN or +infinite sum never wins)
 *   rule 1        m exists and rule 0 does not apply: the pair is m
 *   rule 0 (keep) m exists, prev_pair is given with both entries >= 0, feasible(prev) holds and
 *                 S(m) >= 0.9 * S(prev) (one rounded multiply): the pair is prev_pair. A NaN S(prev) fails the
 *                 comparison: the deliberate difference from the reference of pmaf_select_clear
 *   rule 2 (fallback) no m: with single rounded subtractions ga = c_a[i] - obstacle_margin, gb = c_b[j] -
 *                 obstacle_margin (absent for tracks), gp = clearance(i,j) - pair_margin and
 *                 g = ga; if (gb < g) g = gb; if (gp < g) g = gp;  -- the worst excess over its own margin -- the pair
 *                 of greatest g, strict `>` from -infinity in row-major order. A pair with a NaN gp does not take part
 *   rule -1       rule 2 found nothing: pair = (-1, -1), costs, clearances and worst_excess NaN, first_violation and
 *                 steps -1, nothing adopted
 * prev_pair [2] or NULL; an entry outside [-1, N) -- [-1, n_tracks) for the tracks side -- is PMAF_ERR_INVALID.
 * Outputs. pair [2] is required, every other pointer may be NULL. *n_feasible = the number of feasible pairs; n_clear
 * [2] = the numbers of clear agents per side (tracks: n_tracks); *pair_cost = S and *pair_clearance = clearance of the
 * returned pair; obstacle_clearance [2] and first_violation [2] = c and fv of its two members (tracks: +infinity and
 * the track's window); *worst_excess = g of the returned pair, computed as above whatever the rule; pair_steps [2] = the
 * matrix entry's (step, step) or (step_a, step_b).
 * State. With adopt == 0 the call changes no planner state and the list does not become the resident live list. With
 * adopt != 0 and a pair other than (-1, -1), pop_a adopts i and pop_b adopts j exactly as pmaf_adopt_best would (tracks:
 * only pop adopts); other populations are left alone either way. Waiting, the abandoned-tick refusal (PMAF_ERR_STATE
 * until pmaf_stop) and range checks follow pmaf_select_clear; pop_a == pop_b or an index outside [0, P), n_tracks <= 0
 * and a track count outside [0, cap] are PMAF_ERR_INVALID as in the cross audit. Intended tick:
 *   pmaf_stop -> pmaf_evaluate -> pmaf_select_pair_clear(adopt = 1) -> pmaf_move_real(agent_id = pair) -> pmaf_reset_agents -> pmaf_start */
int pmaf_select_pair_clear(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles, double obstacle_margin,
                           int32_t horizon, int32_t skip_trailing, double separation, double pair_margin, const int32_t *late,
                           const int32_t *prev_pair, int32_t adopt, int32_t *pair, int32_t *rule, int32_t *n_feasible,
                           int32_t *n_clear, double *pair_cost, double *pair_clearance, double *obstacle_clearance,
                           int32_t *first_violation, double *worst_excess, int32_t *pair_steps);
int pmaf_select_clear_tracks(pmaf_planner *h, int32_t pop, const double *obstacles, double obstacle_margin, int32_t horizon,
                             int32_t skip_trailing, int32_t n_tracks, const double *tracks, const int32_t *n_track_points,
                             const double *track_cost, double separation, double pair_margin, const int32_t *late,
                             const int32_t *prev_pair, int32_t adopt, int32_t *pair, int32_t *rule, int32_t *n_feasible,
                             int32_t *n_clear, double *pair_cost, double *pair_clearance, double *obstacle_clearance,
                             int32_t *first_violation, double *worst_excess, int32_t *pair_steps);

/* ---- repulsive track: rollouts that follow the other arm's predicted path (exports added under ABI 7) ----
 * A rollout sees the trailing repulsive obstacle on the straight line o_M + k v_M dt. The audits above can report that
 * the other arm will not be there; nothing above lets a rollout plan around where it WILL be. A population p may
 * therefore have a track y_0 ... y_{L-1}, L >= 1. While it has one, every rollout of p changes repelForce
 * (B/src/cf_agent.cpp:159-181) in one way: at step k (k = 0 is the step from the start state) the obstacle's position
 * is y_{min(k, L-1)} -- the cross audit's hold rule -- instead of the iterated o_M + k v_M dt. Nothing else changes:
 * the radius is the list's radius; the field obstacles advance by predictObstacles; the trailing obstacle's velocity
 * is not used (repelForce reads none); scoring, the real step and pmaf_move_real see the live list as ever; known[M]
 * is carried through. L == 0: no track, the population behaves exactly as without these calls. A track equal to the
 * iterated straight line gives bit-identical rollouts. Points of index >= max_prediction_steps are never read. No
 * reference equivalent. Tracks are inputs, not planner state: pmaf_save_state blobs do not hold them.
 * Known limit: coupled arms each follow the other's PREVIOUS selection, so two arms can alternate between two
 * answers; pmaf_select_pair_clear's hysteresis (rule 0) is the damper.
 * Route. The variant that follows a track exists for the one-slot wave-per-agent kernel of the default arithmetic
 * policy (<= 60 field obstacles, both ordered sums, PLAIN and general step; not the priority-slicing loop of handles
 * with more waves than SIMDs). On any other route a track is never silently ignored: pmaf_set_repulsive_track /
 * pmaf_couple_tracks return PMAF_ERR_STATE with a message naming the route, and so do pmaf_start / pmaf_tick when the
 * route became unsupported after the attach.
 * pmaf_set_repulsive_track: track [P][max_len][3], len [P]; takes effect from the next pmaf_start / pmaf_tick.
 *   track == NULL, len == NULL or every len == 0 detaches. A point inside len that is NaN or outside the supported
 *   numeric range, len < 0 or len > max_len: PMAF_ERR_INVALID. Waits for a running rollout as the setters do; the upload
 *   runs in stream order on the handle's stream into a grow-only device buffer.
 * pmaf_couple_tracks: src_pop [P], -1: none. In front of every rollout launch of this handle, population p with
 *   src_pop[p] = q >= 0 gets as its track the selected path of q -- the path of agent best_idx[q] as it lies in the path
 *   buffer after the tick's selection and before the rollout overwrites it -- from point `shift` >= 0 on:
 *   L = max(n_points - shift, 1) (a path of no more than shift points: its last point alone), the last point held. While
 *   q has no selection yet (no pmaf_evaluate / pmaf_tick so far) L = 0. q == p or q >= P: PMAF_ERR_INVALID. NULL
 *   uncouples. A coupling and an uploaded track on the same population: the coupling wins while it is set. In the
 *   five-call tick pmaf_reset_agents cuts every path to its first point before pmaf_start launches the rollout: on a
 *   coupled handle it takes the selected paths first (after pmaf_adopt_best, if the caller adopts), and the rollout
 *   pmaf_start launches follows those; pmaf_set_initial_position discards what was taken, and so does a call of
 *   pmaf_couple_tracks (the launch then takes from the paths as they lie: after a reset, their first point). An upload
 *   (pmaf_set_repulsive_track) between pmaf_reset_agents and pmaf_start changes the uncoupled populations' tracks only:
 *   what was taken for the coupled ones stays and is followed. Coupled
 *   handles launch one small copy kernel between the manager kernel and the rollout; others keep the two-launch tick.
 * pmaf_get_repulsive_track: the tracks the last launched rollout used (waits for it): len [P], and -- track != NULL --
 *   track [P][max_len][3]; PMAF_ERR_INVALID when max_len is shorter than one of them. An uploaded population shows
 *   what is attached now, cut to max_prediction_steps points. A coupled population shows L = 0 from a call of
 *   pmaf_set_repulsive_track / pmaf_couple_tracks until its track is taken again, and between pmaf_reset_agents and
 *   pmaf_start already the track taken for the launch to come. */
int pmaf_set_repulsive_track(pmaf_planner *h, const double *track, const int32_t *len, int32_t max_len);
int pmaf_couple_tracks(pmaf_planner *h, const int32_t *src_pop, int32_t shift);
int pmaf_get_repulsive_track(pmaf_planner *h, double *track, int32_t *len, int32_t max_len);

/* ---- obstacle tracks: rollouts that follow predicted tracks of the field obstacles (exports added under ABI 7) ----
 * A rollout sees every circular-field obstacle on the straight line o_i + k v_i dt (predictObstacles,
 * B/src/cf_agent.cpp:270-276). A sphere that turns round, a tracked human arm, the links of the other arm along its
 * selected path all leave that line. A population p may therefore have obstacle tracks: L >= 1 points, each point the
 * state of all M field obstacles -- six doubles per obstacle: position, velocity -- and an offset first >= 0. While it
 * has them, every rollout of p changes in one way: at prediction step k (k = 0 is the step from the start state) field
 * obstacle i has the position AND the velocity of point min(first + k, L-1), both taken verbatim and both held at the
 * end, instead of the iterated o_i + k v_i dt with the constant v_i. Nothing else changes: the radii are the creation
 * list's radii; the trailing obstacle stays on its line, or on its repulsive track if the population has one (the two
 * kinds of track may be attached together); the latch, known, min_obs_dist, scoring, the real step, pmaf_move_real, the
 * stepping API and the audits see the live list as ever. L == 0: no tracks, the population behaves exactly as without
 * these calls. Tracks whose points are the iterated straight lines with the constant velocities give bit-identical
 * rollouts. Points of index >= first + max_prediction_steps are never read. No reference equivalent. Tracks are
 * inputs, not planner state: pmaf_save_state blobs do not hold them.
 * Route. As for the repulsive track: the variant that follows obstacle tracks (k_rollout_w64_ftrack, which also follows
 * a repulsive track) exists for the one-slot wave-per-agent kernel of the default arithmetic policy. On any other
 * route pmaf_set_obstacle_tracks returns PMAF_ERR_STATE with a message naming the route, and so do pmaf_start /
 * pmaf_tick when the route became unsupported after the attach. A handle with only a repulsive track, and every
 * handle without tracks, launches what it launched before these calls existed.
 * Limits: no tracks on the multi-slot (> 60 field obstacles), multi-wave, group, sliced and generic routes, nor under
 * the other arithmetic policies; pmaf_evaluate_paths_tracked and pmaf_select_clear_tracked (below) audit and select
 * against the tracks, and pmaf_select_pair_clear_tracked / pmaf_cross_audit_attached (further below) pick and audit the
 * pair against them and against the spheres a coupling attaches; every other audit and selection -- pmaf_evaluate_paths,
 * pmaf_evaluate_path, pmaf_select_clear, pmaf_cross_audit and the slacked cross audits, pmaf_select_pair_clear and
 * pmaf_select_clear_tracks -- keeps the live list's straight lines and does not see them; the planner node
 * (planner_node.h) does not use them.
 * pmaf_set_obstacle_tracks: tracks [P][max_len][M][6] (M = n_obstacles - 1; x y z vx vy vz), len [P]; takes effect from
 *   the next pmaf_start / pmaf_tick and stays until replaced; every population's offset becomes 0. tracks == NULL,
 *   len == NULL or every len == 0 detaches. A value inside len that is NaN or outside the supported numeric range,
 *   len < 0 or len > max_len: PMAF_ERR_INVALID. Waits for a running rollout as the setters do; the upload runs in
 *   stream order on the handle's stream into a grow-only device buffer (transposed on the host so that a wave's load
 *   of one component is contiguous). Tracks that already lie in device memory -- a predictor's output on the same
 *   GPU, float64 or float32, with or without velocities -- go in through pmaf_set_obstacle_tracks_device (further
 *   below) without the trip through the host.
 * pmaf_set_obstacle_track_offset: first [P], each >= 0 (PMAF_ERR_INVALID otherwise): a closed loop that advances
 *   along the same prediction by one point per tick uploads P integers instead of the tracks. PMAF_ERR_STATE while no
 *   tracks are attached.
 * pmaf_get_obstacle_tracks: what the last launched rollout used (waits for it): len [P], first [P] (may be NULL) and
 *   -- tracks != NULL -- tracks [P][max_len][M][6]; PMAF_ERR_INVALID when max_len is shorter than one of them. For a
 *   coupled population (below) that is what the last launched rollout was composed: len = max_prediction_steps (0
 *   before the first composed launch and while no source has a selection), first = 0.
 * pmaf_couple_obstacle_tracks: the device-side source of the tracks -- field obstacles that ride on ANOTHER population's
 *   selected path (the other arm's gripper, its carried object, spheres along its forearm), without the host round trip
 *   of reading that path back and uploading tracks every tick. src_pop [P][M], scale [P][M], anchor [P][M][3].
 *   src_pop[p][i] = q >= 0 attaches field obstacle i of population p to the selected path of population q, -1 attaches
 *   nothing; a population with at least one attached column is COUPLED. src_pop == NULL uncouples everything.
 *   Source path. In front of every rollout launch the selected path of each source q is taken exactly as
 *   pmaf_couple_tracks takes it: the path of agent best_idx[q] as it lies in the path buffer after the tick's selection
 *   (after pmaf_adopt_best, if the caller adopts) and before the rollout overwrites it, from point `shift` on -- with n
 *   that path's n_points clamped to [1, max_prediction_steps], y_0 is its point min(shift, n - 1) and n_c = max(n - shift,
 *   1) --; at pmaf_reset_agents in the five-call tick, otherwise at the launch; pmaf_set_initial_position discards what
 *   was taken, and so does a call of pmaf_couple_obstacle_tracks. While q has no selection yet its columns count as
 *   unattached; if that holds for every attached column of
 *   p, p has L = 0 and rolls out untracked.
 *   Composed tracks. Otherwise a coupled population gets L = max_prediction_steps points and offset 0:
 *     attached column i, k < n_c:   position x_k = RN(anchor + RN(scale * y_k)) per component (one rounded multiply, one
 *                                   rounded add, no contraction);
 *     attached column i, k >= n_c:  position x_{n_c - 1};
 *     attached column, velocity:    u_k = RN(RN(x_{k+1} - x_k) / dt) per component for k < n_c - 1, with dt the handle's
 *                                   rollout step and the correctly rounded division; +0.0 from k = n_c - 1 on;
 *     unattached column:            the iterated straight line of the untracked rollout: q_0 the rollout-start list's
 *                                   position, q_{k+1} = RN(q_k + RN(v dt)), velocity the list's constant v, for all L
 *                                   points (composed at the launch, after the reset has written the rollout-start list);
 *     columns >= M:                 zero.
 *   scale = 1, anchor = 0: the obstacle IS the other end effector; anchor = d: a sphere rigidly attached to it;
 *   scale = s, anchor = (1 - s) base: a point on the segment base -> end effector, a crude link sphere.
 *   Unchanged: the radii, the trailing obstacle (line or repulsive track; both couplings may be on together), the latch,
 *   scoring, the real step -- which still reads the live list, so the caller keeps those rows sensible -- and the
 *   stepping API.
 *   Uploaded tracks and the offset -- nothing is silently ignored: coupling a population that has uploaded tracks
 *   (len > 0) is PMAF_ERR_STATE; pmaf_set_obstacle_tracks with len[p] > 0, or pmaf_set_obstacle_track_offset with
 *   first[p] != 0, for a coupled p is PMAF_ERR_INVALID. Uncoupled populations of the same handle keep their uploaded
 *   tracks and offsets (the shared device buffer's stride becomes max(upload max_len, max_prediction_steps)).
 *   pmaf_evaluate_paths_tracked / pmaf_select_clear_tracked on a coupled population read the tracks the LAST LAUNCHED
 *   rollout followed (the same buffer; nothing newer exists before the next launch), the caller's `first` says how
 *   many ticks have passed; before the first composed launch L = 0, the untracked result.
 *   Route as above: PMAF_ERR_STATE with the route's name at the attach, and from pmaf_start / pmaf_tick after a
 *   reroute. PMAF_ERR_INVALID: q == p, q >= P, q < -1, shift < 0, a NaN or out-of-range scale / anchor entry, scale or
 *   anchor NULL while src_pop is not. Waits and drains like pmaf_couple_tracks. Couplings are inputs, not planner
 *   state: the checkpoint blob does not hold them. Coupled handles launch two small kernels more per tick
 *   (k_fcouple_take, k_fcouple_compose); a handle that never calls this launches exactly what it launched before.
 *   Limits that remain: the joint selection with tracks from the caller (pmaf_select_clear_tracks), the slacked cross
 *   audits and the C++ facade still see straight lines and the end effectors only (pmaf_select_pair_clear_tracked and
 *   pmaf_cross_audit_attached, below, see the tracks and the attached spheres); no tracks on the multi-slot, multi-wave,
 *   group, sliced and generic routes; the planner node does not use them. */
int pmaf_set_obstacle_tracks(pmaf_planner *h, const double *tracks, const int32_t *len, int32_t max_len);
int pmaf_set_obstacle_track_offset(pmaf_planner *h, const int32_t *first);
int pmaf_get_obstacle_tracks(pmaf_planner *h, double *tracks, int32_t *len, int32_t *first, int32_t max_len);
int pmaf_couple_obstacle_tracks(pmaf_planner *h, const int32_t *src_pop /* [P][M] */, const double *scale /* [P][M] */,
                                const double *anchor /* [P][M][3] */, int32_t shift);

/* ---- obstacle tracks from device memory: a predictor on the same device feeds the rollouts (export added under ABI 7) ----
 * pmaf_set_obstacle_tracks takes host memory: a motion predictor that runs on the handle's device would read its output
 * back, widen it to double, invent velocities it may not have, and upload it again, every tick. This call takes the
 * tracks where they lie. Everything it does not restate below is pmaf_set_obstacle_tracks: effect from the next
 * pmaf_start / pmaf_tick until replaced, every offset becomes 0, the route rule and its message (PMAF_ERR_STATE off the
 * one-slot wave-per-agent kernel of the default policy), the coupled-handle rules (a coupled population needs len == 0;
 * the uncoupled populations of a coupled handle are replaced one at a time; a buffer that must grow keeps what it holds;
 * stride max(upload max_len, max_prediction_steps)), columns >= M zero, every len == 0 detaches, tracks are inputs and
 * not checkpoint state, and pmaf_get_obstacle_tracks returns the ingested points -- with components == 3 the derived
 * velocities too. Detaching with NULL stays the host call's business: pmaf_set_obstacle_tracks(h, NULL, NULL, 0).
 * Source. d_tracks: memory the handle's device can read (device memory of that device, of a peer device with peer
 *   access, pinned or managed host memory), [P][max_len][M][components] elements of `dtype`, densely packed,
 *   M = n_obstacles - 1. Of population p exactly the leading len[p] * M * components elements of its slab are read; what
 *   lies in the padding up to max_len is neither read nor validated (as in the host call). Alignment is the element's
 *   own, 8 bytes for PMAF_TRACK_F64 and 4 for PMAF_TRACK_F32 (less: PMAF_ERR_INVALID); a source that is 8-aligned but not
 *   16-aligned is legal. len stays a HOST array of P integers.
 * components == 6: position and velocity, taken verbatim: PMAF_TRACK_F32 is widened to double exactly, the bit pattern
 *   of a PMAF_TRACK_F64 value is preserved (-0.0 included) -- with F64 this is pmaf_set_obstacle_tracks on the same
 *   numbers, bit for bit.
 * components == 3: positions only, taken as above (F32 widened first; differences and quotients in double). The
 *   velocity of point k < len - 1 is u_k = RN(RN(x_{k+1} - x_k) / dt) per component, dt the handle's rollout step, the
 *   division the correctly rounded one, no contraction; +0.0 at point len - 1, which the rollout holds: a held obstacle
 *   rests. (The composed tracks' velocity rule of pmaf_couple_obstacle_tracks, for uploaded positions.)
 * Validation, on the device: every ingested value -- after widening, and with components == 3 every derived velocity
 *   as well -- is finite and either 0 or 2^-100 <= |x| <= 2^100 (an F32 subnormal is refused, and dt == 0 refuses
 *   itself). A violation is PMAF_ERR_INVALID with a message that names population, point, obstacle and component (0 .. 2
 *   position, 3 .. 5 velocity) of the FIRST offender in source order, decided by a minimum over a flat index: a derived
 *   velocity counts at its point, behind its obstacle's positions, and is judged only where both positions it is taken
 *   from pass themselves (an out-of-range position is named itself, not through the difference it spoils). A refused
 *   call changes nothing: tracks, lengths, offsets and route stay, pmaf_get_obstacle_tracks returns what it returned.
 * Other arguments. d_tracks == NULL, len == NULL, max_len < 1, len[p] outside [0, max_len], components not 3 or 6, an
 *   unknown dtype: PMAF_ERR_INVALID. The pointer is classified before anything is enqueued (hipPointerGetAttributes):
 *   pageable host memory and another device's memory without peer access are PMAF_ERR_INVALID (enabling peer access is
 *   the caller's: the call leaves the process's device state as it finds it), and so is, where the runtime can tell
 *   (hipMemGetAddressRange), a source whose last element to be read lies outside its allocation.
 * Ordering. producer_stream != NULL (a hipStream_t of the handle's device): the ingest waits for everything enqueued on
 *   that stream up to the call -- an event recorded there, awaited by the handle's stream; the producer is never
 *   synchronised with the host. NULL: the caller vouches that the data is complete, or produced it on pmaf_stream(h).
 *   Waits for a running rollout as the setters do (it still reads the buffer), refuses an abandoned tick as they do,
 *   and returns after the ingest has finished: the source may be overwritten on return, and there is one set of tracks.
 * Cost. Two small kernels per call (k_ftingest_check, k_ftingest_store: the second returns at once behind a refusal)
 *   and one 8-byte copy for the verdict; a handle that never calls this launches exactly what it launched before.
 * Out of scope: a device source for the repulsive track and for the live obstacle list; an asynchronous form whose
 *   verdict arrives at the next launch; tracks on the routes that refuse them (Limits above). */
#define PMAF_TRACK_F64 0
#define PMAF_TRACK_F32 1
int pmaf_set_obstacle_tracks_device(pmaf_planner *h, const void *d_tracks, const int32_t *len /* host, [P] */,
                                    int32_t max_len, int32_t components /* 6 or 3 */, int32_t dtype,
                                    void *producer_stream /* hipStream_t, or NULL */);

/* ---- audits against the obstacle tracks: the path audit and the clear selection where the rollouts saw the field
 * obstacles (exports added under ABI 7) ----
 * On a handle with obstacle tracks the rollout bends its paths round the predicted positions, while pmaf_evaluate_paths
 * and pmaf_select_clear hold every path against the list's straight lines: a path bent round a predicted turn is
 * rejected where the line cuts through it, and a path through the place the obstacle turns into is selected as clear.
 * These two calls are exactly pmaf_evaluate_paths' and pmaf_select_clear's contracts with ONE change, the position of a
 * tracked field obstacle. For population p let L = len[p] be the length of the tracks attached NOW -- what the next
 * rollout launch would follow; the setters synchronise, so there is one set of tracks; for a population coupled with
 * pmaf_couple_obstacle_tracks the tracks the LAST LAUNCHED rollout followed, L = 0 before the first composed launch:
 * the next launch's are composed only in front of it --, f = first[p] when first is
 * given, else the handle's current offset of p, and M = n_obstacles - 1.
 *   tracked field obstacle (L > 0, j < M):  o_j^k = the POSITION of track point min(f + k, L-1), taken verbatim and held
 *              at the end -- the rollout's rule: step k from x_k sees point min(first + k, L-1). The track's velocities
 *              are not read. f may be as large as INT32_MAX: min(f + k, L-1) = min(min(f, L-1) + k, L-1), and the
 *              right-hand side is what is computed.
 *   trailing obstacle (j = M):              stays on the list's iterated line o^{k+1} = o^k + RN(v dt), as in the
 *              untracked calls (it does not follow a repulsive track either). pmaf_evaluate_paths_tracked always
 *              includes it; pmaf_select_clear_tracked leaves it out when skip_trailing != 0 (the joint selection's
 *              convention: obstacles 0 .. n_obstacles - 2 of every list are audited).
 *   untracked population (L == 0):          every obstacle is on the list's line: the result is bit for bit that of
 *              the untracked call.
 *   radii:     radius + r_j with r_j from the CALLER'S list, as in the untracked audits -- NOT the creation list's radii
 *              the rollout uses.
 * Unchanged: the window w = min(n, horizon), the strict `<` from +infinity, the tie rules (smallest k, then smallest j,
 * across tracked and trailing obstacles alike), first_violation, per_obstacle, the rules 0 / 1 / 2 with the 0.9
 * hysteresis, the outputs and which of them may be NULL. adopt works like pmaf_adopt_best. The calls wait for a running
 * rollout, refuse a handle whose tick was abandoned (pmaf_select_clear_tracked; PMAF_ERR_STATE until pmaf_stop), and
 * with adopt == 0 change no planner state: neither the attached tracks nor the handle's offsets move, and a tick
 * sequence with such calls in between is bit-identical to one without.
 * first [P] or NULL. An entry below 0: PMAF_ERR_INVALID. first != NULL on a handle with no tracks attached:
 * PMAF_ERR_STATE, like pmaf_set_obstacle_track_offset. first == NULL on a handle without tracks is allowed and gives the
 * untracked result. Everything else is validated as in the untracked calls.
 * Tracks whose points are the iterated straight lines of the caller's list give bit for bit the untracked results.
 * Intended six-call tick on a tracked handle (CfManager::planTickAudited(..., tracked = true)):
 *   pmaf_stop -> pmaf_evaluate -> pmaf_select_clear_tracked(adopt = 1) -> pmaf_move_real(agent_id = pick)
 *   -> pmaf_reset_agents -> [pmaf_set_obstacle_track_offset] -> pmaf_start */
int pmaf_evaluate_paths_tracked(pmaf_planner *h, const double *obstacles, const int32_t *first, double margin,
                                double *clearance, int32_t *step, int32_t *obstacle, int32_t *first_violation,
                                double *per_obstacle);
int pmaf_select_clear_tracked(pmaf_planner *h, const double *obstacles, const int32_t *first, double margin,
                              int32_t horizon, int32_t skip_trailing, const int32_t *prev_idx, int32_t adopt,
                              int32_t *pick, int32_t *rule, int32_t *n_clear, double *cost, double *clearance,
                              int32_t *first_violation);

/* ---- clear selection with timing slack: an arm that runs late stays clear (exports added under ABI 7) ----
 * Every audit above holds step k of a predicted path against step k of the obstacles, as if both were one instant. On a
 * robot they are not: the real end effector trails its set-points (the closed-loop scenarios run with a 30 % tracking
 * lag), and a motion predictor's clock is not the controller's. The cross audit with timing slack answers that for arm
 * against arm; these two calls answer it for arm against obstacles, which is where the obstacle tracks put a
 * time-indexed prediction into the planner: a path that passes behind a moving obstacle is clear step against step and
 * is hit when the arm is three steps late. No reference equivalent.
 * Carried over unchanged from pmaf_evaluate_paths_tracked and pmaf_select_clear_tracked: the window w (n for the
 * evaluate call, min(n, horizon) for the selection); first ([P] or NULL, clamped to L-1 before anything is added, may be
 * INT32_MAX, an entry below 0 PMAF_ERR_INVALID, first != NULL on a handle without tracks PMAF_ERR_STATE); a population
 * with L == 0, and a handle without tracks, are on the list's iterated line; the trailing obstacle stays on the list's
 * line and is left out with skip_trailing != 0 (the selection only); radius + r_j with r_j from the CALLER'S list; the
 * build's dot association; rules 0 / 1 / 2 with the 0.9 hysteresis; adopt, the wait for a running rollout, the refusal of
 * a handle whose tick was abandoned (the selection; PMAF_ERR_STATE until pmaf_stop), no state change with adopt == 0 (a
 * tick sequence with such calls in between is bit-identical to one without); which outputs may be NULL.
 * The one change: the obstacles have a time index l of their own.
 *   late >= 0:   the arm may be up to `late` steps BEHIND the obstacles' clock: it stands at x_k while they are at index
 *                k + s, 0 <= s <= late.
 *   early >= 0:  the obstacles may be up to `early` steps behind the arm's clock (a predictor that leads, an arm ahead of
 *                schedule): the arm at x_k, they at index k - s, 0 <= s <= early.
 *   admitted:    the pairs (k, l) with 0 <= k < w, l >= 0 and -early <= l - k <= late. l has no upper bound of its own:
 *                obstacles do not end where the path does.
 *   tracked field obstacle (L > 0, j < M) at index l: the POSITION of track point min(min(f, L-1) + l, L-1), taken
 *                verbatim and held at the end (the hold applies to the slacked index, not before the slack is added).
 *   every other obstacle at index l: on the list's chain o^0 = the caller's position, o^{l+1} = o^l + RN(v dt) per
 *                component. The chain is walked from o^0 and never multiplied out: o^l has the bits of
 *                pmaf_evaluate_paths' track for every l, also for l >= w.
 *   c(k,l,j)   = norm(x_k - o_j^l) - (radius + r_j)
 *   clearance_a = the minimum of c over the admitted (k, l) and the audited j under the total order (c, k, l, j): ties go
 *                to the smallest k, then the smallest l, then the smallest j. A NaN never wins and never violates. When
 *                nothing won (an empty window, nothing audited, NaN or +infinity everywhere): +infinity with
 *                (step, obstacle_step, obstacle) = (-1, -1, -1). step = k, obstacle_step = l, obstacle = j.
 *   first_violation_a = the smallest k < w for which some admitted l and audited j have c(k,l,j) < margin, else w. It
 *                reports the ARM'S step, not the obstacles' index.
 * late < 0 or early < 0: PMAF_ERR_INVALID. Values of max_prediction_steps or more are clamped to it on the host, before
 * any device arithmetic: the clamped value is the slack of the call (an `early` of that size already reaches index 0
 * from every point of the window; a `late` of that size is a whole rollout behind). Then l < 2 * max_prediction_steps
 * and no index can overflow.
 * Consequences:
 *   - (late, early) = (0, 0) gives pmaf_evaluate_paths_tracked's and pmaf_select_clear_tracked's outputs bit for bit, with
 *     obstacle_step == step (through this block's own kernel all the same);
 *   - clearance, first_violation and n_clear never grow when either slack grows;
 *   - a list at rest on a handle without tracks gives the unslacked bits for every slack (every index is one place);
 *     obstacle_step is then the band's first index, max(step - early, 0).
 * pmaf_evaluate_paths_slack: clearance [P][N] is required; step, obstacle_step, obstacle, first_violation [P][N] may each
 * be NULL. Every obstacle of the list is audited, the trailing one included. There is no per_obstacle output.
 * pmaf_select_clear_slack: pick [P] is required; rule, n_clear, cost, clearance, first_violation [P] may each be NULL;
 * horizon and prev_idx are validated as in pmaf_select_clear.
 * Cost: every obstacle position is held against late + early + 1 path points instead of one; horizon is the caller's
 * lever at tick rate (profiles/obstacle_slack_audit.md).
 * Out of scope, and so still step against step: per_obstacle, and the obstacle side of the pair selections
 * (pmaf_select_pair_clear and its tracked and slacked forms, pmaf_select_clear_tracks) -- their `late` is the arms' slack
 * against each other only.
 * Intended six-call tick (CfManager::planTickAudited(..., tracked = true, late, early)):
 *   pmaf_stop -> pmaf_evaluate -> pmaf_select_clear_slack(adopt = 1) -> pmaf_move_real(agent_id = pick)
 *   -> pmaf_reset_agents -> [pmaf_set_obstacle_track_offset] -> pmaf_start */
int pmaf_evaluate_paths_slack(pmaf_planner *h, const double *obstacles, const int32_t *first, double margin,
                              int32_t late, int32_t early, double *clearance, int32_t *step, int32_t *obstacle_step,
                              int32_t *obstacle, int32_t *first_violation);
int pmaf_select_clear_slack(pmaf_planner *h, const double *obstacles, const int32_t *first, double margin,
                            int32_t horizon, int32_t skip_trailing, int32_t late, int32_t early,
                            const int32_t *prev_idx, int32_t adopt, int32_t *pick, int32_t *rule, int32_t *n_clear,
                            double *cost, double *clearance, int32_t *first_violation);

/* ---- joint selection on coupled handles: pairs held to the riding spheres (exports added under ABI 7) ----
 * pmaf_couple_obstacle_tracks puts spheres of one arm's list on the OTHER arm's selected path (gripper, load, forearm
 * spheres at anchor + scale * point) and the rollouts bend round them. pmaf_select_pair_clear then picks the pair
 * against the live list's straight lines and holds the two arms against each other at one point per arm: a pair in
 * which arm A's end effector passes through the sphere on arm B's forearm is feasible. These two calls audit a pair
 * (i, j) against the spheres the coupling exists for, riding on the path of the candidate that is being picked -- not on
 * the last launch's selection, which is stale for it. No reference equivalent.
 * Terms of a pair. a = pop_a, b = pop_b, M = n_obstacles - 1; src_pop, scale, anchor = the handle's CURRENT coupling,
 * what pmaf_couple_obstacle_tracks last set (nothing attached on a handle that is not coupled); `shift` is NOT used:
 * step k of both candidate paths is one instant, as in the cross audit. S_ab = {s < M : src_pop[a][s] == b}, the spheres
 * of A's list that are parts of arm B; S_ba = {s < M : src_pop[b][s] == a}. xh, yh, K = max(n, m), the hold rule and the
 * empty-path rule are pmaf_cross_audit's. The terms, in this order:
 *   term 0:                          the end effectors: u = xh_k, z = yh_k, R_0 = separation
 *   term 1 + s, s in S_ab ascending: u = xh_k, z = RN(anchor[a][s] + RN(scale[a][s] * yh_k)) per component -- one rounded
 *                                    multiply, one rounded add, nothing fused: the composer's formula --,
 *                                    R = RN(radius + r) with radius = pmaf_params.radius, r = obstacles[a][s][6]
 *   term 1 + M + s, s in S_ba asc.:  u = yh_k, z = RN(anchor[b][s] + RN(scale[b][s] * xh_k)), r = obstacles[b][s][6]
 *   d2_t   = min over k < K of dot(u - z, u - z) in the build's association (pmaf_eval_order), every operation rounded,
 *            strict `<` from +infinity, k ascending; a NaN never wins
 *   gap_t  = sqrt(d2_t) - R_t, +infinity if nothing won
 *   clearance(i,j) = min over t of gap_t, strict `<` from +infinity in term order: ties go to the smallest term, then
 *            the smallest k. step(i,j) = the winning term's k; sphere(i,j) = its code 0, 1 + s or 1 + M + s. Nothing
 *            won, or an empty path: +infinity / -1 / -1. No term has a margin of its own.
 * With S_ab and S_ba empty this is pmaf_cross_audit bit for bit, and sphere is 0 wherever a step won.
 *
 * pmaf_cross_audit_attached: the matrices above on the whole CURRENT paths of pop_a and pop_b. clearance [N][N] is
 * required; step [N][N] and sphere [N][N] may be NULL. obstacles [P][n_obstacles][7] is range-checked like every list;
 * only its radii are read. Waits, state rules (none is changed) and validation are pmaf_cross_audit's.
 *
 * pmaf_select_pair_clear_tracked: pmaf_select_pair_clear's contract with late == NULL -- window, rules -1 / 0 / 1 / 2,
 * S, g, record, adopt, waits, the abandoned-tick refusal, outputs and which of them may be NULL -- with two changes.
 *   Obstacle side. c, fv and clear of both sides are pmaf_select_clear_tracked's with the same first ([P] or NULL, its
 *     validation and its PMAF_ERR_STATE rule), horizon and skip_trailing: a field obstacle of a population with tracks
 *     is where the rollouts saw it. Side A's audit also leaves out the columns of S_ab and side B's those of S_ba:
 *     those spheres ride on the last launch's selection, which is stale for the pair being picked, and the pair side
 *     replaces them, as it replaces the trailing sphere. Columns attached to a third population, and unattached
 *     columns, stay as pmaf_select_clear_tracked has them. If nothing is left to audit, c = +infinity and every agent
 *     is clear.
 *   Pair side. clearance(i,j) and pair_steps = (step, step) are the attached audit's on the two path sets cut to their
 *     windows, held to pair_margin.
 * On a handle without tracks and without coupling the call is pmaf_select_pair_clear(late = NULL) bit for bit, through
 * the same kernels.
 * Limits that remain: pmaf_select_clear_tracks, whose side B comes from the caller, sees neither tracks nor
 * attachments; the C++ facade (one population per handle) uses neither call. Timing slack: the block below. */
int pmaf_cross_audit_attached(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles, double separation,
                              double *clearance, int32_t *step, int32_t *sphere);
int pmaf_select_pair_clear_tracked(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles,
                                   const int32_t *first, double obstacle_margin, int32_t horizon, int32_t skip_trailing,
                                   double separation, double pair_margin, const int32_t *prev_pair, int32_t adopt,
                                   int32_t *pair, int32_t *rule, int32_t *n_feasible, int32_t *n_clear, double *pair_cost,
                                   double *pair_clearance, double *obstacle_clearance, int32_t *first_violation,
                                   double *worst_excess, int32_t *pair_steps);

/* ---- joint selection on coupled handles with timing slack: late arms held to the riding spheres (exports added under
 * ABI 7) ----
 * The slacked calls (pmaf_cross_audit_slack, pmaf_select_pair_slack, pmaf_select_pair_clear(late)) admit every pair of
 * steps in a band but see the two end effectors only; the attached calls above hold a pair to the riding spheres, step
 * against step only. These two calls are their product: every term of a pair over the whole band. No reference
 * equivalent.
 * Carried over unchanged: the terms, their order, S_ab / S_ba, the ride z = RN(anchor + RN(scale * p)), R_0 =
 * separation, R = RN(radius + r) with r from the caller's list and the codes 0, 1 + s, 1 + M + s are
 * pmaf_cross_audit_attached's; xh, yh, K = max(n, m), the hold rule and the empty-path rule are pmaf_cross_audit's; the
 * admitted set is pmaf_cross_audit_slack's: (k, l) in [0, K)^2 with -late_b <= l - k <= late_a. k is ALWAYS A's step
 * and l ALWAYS B's.
 *   term 0:                  u = xh_k, z = yh_l
 *   term 1 + s, s in S_ab:   u = xh_k, z = RN(anchor[a][s] + RN(scale[a][s] * yh_l)): the sphere is a part of arm B and
 *                            is on arm B's clock
 *   term 1 + M + s, S_ba:    u = yh_l, z = RN(anchor[b][s] + RN(scale[b][s] * xh_k))
 *   d2_t   = the least dot(u - z, u - z) over the admitted pairs under the total order (d2, k, l): a scan with k, then l
 *            ascending and a strict `<` from +infinity; a NaN never wins
 *   gap_t  = sqrt(d2_t) - R_t
 *   clearance(i,j) = min over t of gap_t, strict `<` in term order: ties go to the smallest term, then to that term's
 *            least (k, l). (step_a, step_b)(i,j) and sphere(i,j) are the winning term's. Nothing won, or an empty
 *            path: +infinity / -1 / -1 / -1.
 * Consequences:
 *   - late_a = late_b = 0 gives pmaf_cross_audit_attached's clearance and sphere bit for bit, with step_a = step_b =
 *     step (through this call's own kernel all the same);
 *   - with S_ab and S_ba empty the call is pmaf_cross_audit_slack bit for bit, and sphere is 0 wherever a step won;
 *   - the clearance never grows with either slack;
 *   - audit(A, B, late_a, late_b) has the transposed clearance bits of audit(B, A, late_b, late_a): each sphere's u - z is
 *     the same vector in both calls, the codes swap 1 + s <-> 1 + M + s, and the steps transpose only where the minimum
 *     is unique (the tie order (d2, k, l) is not symmetric).
 *
 * pmaf_cross_audit_attached_slack: the matrices above on the whole CURRENT paths of pop_a and pop_b. clearance [N][N] is
 * required; step_a, step_b and sphere [N][N] may each be NULL. A negative slack: PMAF_ERR_INVALID; a slack of
 * max_prediction_steps or more already admits every pair of steps and is clamped on the host. Waits, state rules (none
 * is changed) and every other validation are pmaf_cross_audit_attached's.
 *
 * pmaf_select_pair_clear_tracked_slack: late == NULL is pmaf_select_pair_clear_tracked exactly, through the same
 * kernels. With late [2] = (late_a, late_b): the obstacle side is unchanged; the pair side is the matrix above on the
 * two path sets cut to their windows, held to pair_margin; pair_steps = (step_a, step_b) of the returned pair. Rules
 * -1 / 0 / 1 / 2, S, g, record, adoption, waits, the abandoned-tick refusal, outputs and which of them may be NULL are
 * untouched. Where nothing rides on the other member of the pair the pair side is pmaf_select_pair_clear(late)'s.
 * Limits that remain: pmaf_select_clear_tracks sees neither tracks nor attachments; the C++ facade (one population per
 * handle) and the planner node use none of this. */
int pmaf_cross_audit_attached_slack(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles,
                                    double separation, int32_t late_a, int32_t late_b, double *clearance,
                                    int32_t *step_a, int32_t *step_b, int32_t *sphere);
int pmaf_select_pair_clear_tracked_slack(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles,
                                         const int32_t *first, double obstacle_margin, int32_t horizon,
                                         int32_t skip_trailing, double separation, double pair_margin,
                                         const int32_t *late /* [2] or NULL */, const int32_t *prev_pair, int32_t adopt,
                                         int32_t *pair, int32_t *rule, int32_t *n_feasible, int32_t *n_clear,
                                         double *pair_cost, double *pair_clearance, double *obstacle_clearance,
                                         int32_t *first_violation, double *worst_excess, int32_t *pair_steps);

/* CfManager::getLinkForce -> CfAgent::bodyForce, B/src/cf_manager.cpp:169-182,
 * B/src/cf_agent.cpp:229-234: repel-only force of population `pop`'s last
 * obstacle at n link points. link_pos [n][3], k_r_force [n], out [n][3]. */
int pmaf_link_force(pmaf_planner *h, int32_t pop, int32_t n,
                    const double *link_pos, const double *k_r_force,
                    const double *obstacles, double *out);

/* ---- getters ---- */
/* Getters of rollout results (paths, costs, lengths, distances, flags,
 * rotation vectors) wait for the running rollout; the real-agent getters
 * (pmaf_get_real_state, pmaf_get_dist_from_goal, pmaf_get_real_path) are served
 * from host copies and return at once, like the reference's. */
/* getPredictedPaths / getNumPredictionSteps: paths [P][N][cap][3], n_points [P][N] */
int pmaf_get_paths(pmaf_planner *h, double *paths, int32_t *n_points);
/* The same data without the copy: *paths [P][N][cap][3] (entries past a path's
 * end are zero) and *n_points [P][N] point into the handle's pinned host mirror,
 * refreshed by ONE device-to-host copy per rollout generation however often the
 * getters are called (the reference's node calls getPredictedPaths() 3 x N
 * times per tick, B/src/panda_bimanual_control.cpp:341-344). Valid until the
 * next call that changes the predicted paths (start / tick / reset / set_* /
 * move_agents / load_state / attach). Either pointer may be NULL. */
int pmaf_view_paths(pmaf_planner *h, const double **paths, const int32_t **n_points);
/* costs of the last pmaf_evaluate / pmaf_tick, [P][N] */
int pmaf_get_costs(pmaf_planner *h, double *costs);
/* getPredictedPathLengths, B/src/cf_manager.cpp:192-198, [P][N] */
int pmaf_get_path_lengths(pmaf_planner *h, double *out);
/* CfAgent::getMinObsDist, [P][N] */
int pmaf_get_min_obs_dist(pmaf_planner *h, double *out);
/* getAgentSuccess, B/src/cf_manager.cpp:208-214, [P][N] (0/1): written by a rollout for the agents that took a step in
 * it (B/src/cf_agent.cpp:330-337); a reset, a restart of the paths and a rollout in which the agent took no step leave
 * the flag of the last rollout in which it did */
int pmaf_get_success(pmaf_planner *h, int32_t *out);
/* CfAgent::getVelocity of every predicted agent, [P][N][3] */
int pmaf_get_agent_velocities(pmaf_planner *h, double *out);
/* field_rotation_vecs_ [P][N][n_obstacles][3] and known_obstacles_ [P][N][n_obstacles] */
int pmaf_get_rotation_vectors(pmaf_planner *h, double *rot, int32_t *known);
/* getNextPosition / getNextVelocity / getEEForce (cf_manager.h:74-79), each [P][3], may be NULL */
int pmaf_get_real_state(pmaf_planner *h, double *pos, double *vel, double *force);
/* RealCfAgent known_obstacles_ [P][n_obstacles], field_rotation_vecs_ [P][n_obstacles][3] */
int pmaf_get_real_known(pmaf_planner *h, int32_t *known, double *rot);
/* getPlannedTrajectory (cf_manager.h:90-92) of population pop: copies up to
 * max_points points into out [max_points][3]; *n_total = path size. */
int pmaf_get_real_path(pmaf_planner *h, int32_t pop, double *out,
                       int32_t max_points, int32_t *n_total);
/* getDistFromGoal (cf_manager.h:87-89), [P] */
int pmaf_get_dist_from_goal(pmaf_planner *h, double *out);
/* getBestAgentType (cf_manager.h:73): type [P] (-1 = none yet), id [P] 1-based (0 = none) */
int pmaf_get_best(pmaf_planner *h, int32_t *type, int32_t *id);
/* getPredictionTimes (B/src/cf_manager.cpp:200-206; CfAgent::prediction_time_,
 * B/src/cf_agent.cpp:308-331): duration of each agent's last rollout in ns,
 * [P][N], from the device's constant-rate clock (wall_clock64) read by the
 * agent's wave at the start and the end of its rollout. */
int pmaf_get_prediction_times_ns(pmaf_planner *h, double *out);

/* ---- state transfer / sharding support (no reference equivalent) ---- */
/* restore hysteresis reference (best_agent_ survives CfManager::init): id
 * 1-based [P] (0 = none), type [P], rand [P][n_obstacles][3] */
int pmaf_set_best(pmaf_planner *h, const int32_t *id, const int32_t *type,
                  const double *rand_vecs);
/*
 * Winner record of a population = the result of its last selection
 * (pmaf_evaluate / pmaf_tick): PMAF_WINNER_RECORD_HEADER doubles
 *   {cost, agent index, n_points, agent type, real agent's position[3] (the
 *    set-point just published), its distance from the goal}
 * followed by the selected agent's predicted path[cap][3] (the path that was
 * scored; entries past n_points are zero) = (8 + 3*cap) doubles.
 * pmaf_write_winner_records packs the records of all P populations into DEVICE
 * memory `dst` on the handle's stream (call it after pmaf_evaluate, before
 * the agents are reset; pmaf_stop() or a stream-ordered consumer makes it
 * visible).
 */
#define PMAF_WINNER_RECORD_HEADER 8
int pmaf_write_winner_records(pmaf_planner *h, void *dst_device, size_t bytes);
size_t pmaf_winner_record_doubles(const pmaf_planner *h);
/* the hipStream_t the handle launches on (as void*), for stream-ordered consumers */
void *pmaf_stream(pmaf_planner *h);

/* ---- multi-GPU: one process per GPU, populations sharded over ranks ----
 * The path shards by POPULATION: every rank plans its own populations with its
 * own handle and there is no collective on the rollout's data path. Where a
 * run needs every population's winning trajectory on every rank (the dual-arm
 * coupling of BASELINE config 4, a goal sweep's global pick) the fixed-size
 * winner records are exchanged with ONE all-gather per tick -- RCCL
 * (ncclAllGather over xGMI) between GPUs. No reference equivalent: the
 * reference is a single-process CPU planner. */
typedef struct pmaf_comm pmaf_comm;
#define PMAF_COMM_ID_BYTES 128
/* ncclGetUniqueId: call on ONE rank and hand the 128 bytes to every rank
 * (MPI, a file, a socket, torch.distributed ...). */
int pmaf_comm_unique_id(void *id_out);
/* ncclCommInitRank on HIP device `device` (-1 = current device); collective
 * over all `world` ranks. */
int pmaf_comm_init_rccl(int32_t world, int32_t rank, const void *id, int32_t device, pmaf_comm **out);
/* wrap an ncclComm_t the caller already owns (not destroyed by
 * pmaf_comm_destroy), e.g. the communicator of a host application */
int pmaf_comm_from_rccl(void *nccl_comm, int32_t device, pmaf_comm **out);
/* Host-transport communicator (MPI, gloo, tests): `fn` must all-gather
 * bytes_per_rank bytes of HOST memory of every rank into recv (rank-major)
 * and return 0. Records are staged through pinned host memory. */
typedef int (*pmaf_host_allgather_fn)(void *ctx, const void *send, void *recv, size_t bytes_per_rank);
int pmaf_comm_init_host(int32_t world, int32_t rank, pmaf_host_allgather_fn fn, void *ctx, pmaf_comm **out);
int pmaf_comm_destroy(pmaf_comm *c);
int pmaf_comm_world(const pmaf_comm *c);
int pmaf_comm_rank(const pmaf_comm *c);
/* blocking all-gather of n_per_rank doubles of HOST data per rank (small
 * control-plane exchanges: agent-range cost vectors, set-points). */
int pmaf_comm_allgather(pmaf_comm *c, const double *send, double *recv, size_t n_per_rank);
/* CfManager::evaluateAgents' selection rule (B/src/cf_manager.cpp:336-353) on
 * a cost vector gathered from agent-range shards: first minimum, then the 0.9
 * hysteresis against prev_best (global 0-based index, -1 = none). */
int32_t pmaf_select_best(const double *costs, int32_t n, int32_t prev_best);

/* One-shot exchange: pmaf_write_winner_records into an internal send buffer,
 * then the all-gather of all ranks' P records into DEVICE memory recv_device
 * [world][P][record] -- with an RCCL communicator both are enqueued on the
 * handle's stream with no host synchronisation in between (pmaf_stop() or a
 * stream-ordered consumer makes the result visible); a host communicator
 * blocks. Same call-time rule as pmaf_write_winner_records. */
int pmaf_allgather_winners(pmaf_planner *h, pmaf_comm *c, void *recv_device, size_t bytes);
/* Per-tick exchange for the fused tick: once a communicator is attached,
 * every pmaf_tick / pmaf_evaluate publishes the winner records of its
 * selection and all-gathers them on a second stream while the next rollout
 * runs (the handle then keeps two path buffers so the rollout cannot overwrite
 * the path being sent). c = NULL detaches. The communicator must outlive the
 * attachment. */
int pmaf_attach_comm(pmaf_planner *h, pmaf_comm *c);
/* (The handle keeps two exchange slots: a tick never waits for the collective
 * of the tick before it, only -- when it comes to reuse that slot -- for the
 * one two ticks back.)
 * wait for the exchange of the last pmaf_tick / pmaf_evaluate; *records =
 * [world][P][record] doubles in pinned host memory, valid until the next
 * pmaf_tick / pmaf_evaluate; *n_doubles = world * P * record. */
int pmaf_winners_wait(pmaf_planner *h, const double **records, size_t *n_doubles);
/* device copy of the same table (valid after pmaf_winners_wait) */
void *pmaf_winners_device(pmaf_planner *h);
/* duration of the completed exchanges' all-gathers in microseconds (device
 * time between the events around ncclAllGather, i.e. including the wait for
 * the slowest rank; host communicator: wall time of the callback), oldest
 * first, at most max_n; *n = number written. Clears the record. */
int pmaf_get_exchange_times_us(pmaf_planner *h, double *out, int32_t max_n, int32_t *n);
/* host-side clock of the newest pmaf_tick calls (at most 8192 are kept), oldest first, in microseconds from the call's
 * entry: enqueue_us = both launches (k_manager, rollout) handed to the stream, setpoint_us = best index + next
 * set-point on the host (what the reference's planCallback publishes, B/src/panda_bimanual_control.cpp:329-369;
 * the rollout keeps running behind it). Either array may be NULL; *n = number written; clears the record.
 * Measured inside the library, so a caller in an interpreted language sees the path's latency, not its own. */
int pmaf_get_tick_times_us(pmaf_planner *h, double *enqueue_us, double *setpoint_us, int32_t max_n, int32_t *n);

/* ---- peer mailboxes: header-only exchange WITHOUT a collective (ABI 3) ----
 * Where a population needs only another population's set-point of the previous
 * tick (BASELINE config 4: each arm's trailing repulsive obstacle is the other
 * arm's end effector, B/src/cf_agent.cpp:159-181 for the obstacle's role), a
 * collective per tick puts a launch + rendezvous on the control path. Instead
 * every rank owns an INBOX in its device memory that is mapped into every peer
 * process (hipIpcGetMemHandle / hipIpcOpenMemHandle; peer GPUs reach it over
 * xGMI). The manager kernel of pmaf_tick number t
 *   - stores the 8-double record header of each of its populations, then the
 *     sequence number t behind a system-scope release, straight into slot
 *     [t & 1][rank][pop] of EVERY rank's inbox, and
 *   - for a population coupled with pmaf_peer_couple, reads the header with
 *     sequence number t-1 of (src_rank, src_pop) from its OWN inbox (local HBM)
 *     and uses its position[3] as the live trailing obstacle (velocity 0, the
 *     given radius) of this tick's real step and of the rollout it starts.
 * No host, no stream, no collective is involved; the winner-record all-gather
 * above stays what it was (the path table, off the control path). Every rank
 * must issue the same number of pmaf_tick calls; the other entry points
 * (pmaf_evaluate ...) neither publish nor consume.
 * TOPOLOGY: couplings must be PAIRWISE MUTUAL (population a reads b's header and b reads a's -- the dual-arm case).
 * The two parity slots per source rest on it: a source cannot publish tick t+1 (which overwrites header t-1) before it
 * has read the consumer's header t. A one-way coupling or a ring of three or more has no such back-pressure; the
 * consumer detects it from the coupling the publisher writes into its header and pmaf_tick fails with PMAF_ERR_STATE
 * (likewise when a source is found to have run ahead). Not part of a checkpoint
 * (reconnect after pmaf_load_state). No reference equivalent. */
#define PMAF_PEER_HANDLE_BYTES 128
/* allocate this handle's inbox for `world` ranks and export it: hand the
 * PMAF_PEER_HANDLE_BYTES bytes of every rank to every rank (any transport) */
int pmaf_peer_export(pmaf_planner *h, int32_t world, void *handle_out);
/* handles = [world][PMAF_PEER_HANDLE_BYTES] in rank order (handles[rank] = this
 * handle's own export). Handles exported by the same process are used directly
 * (several handles of one process: one host driving several GPUs, tests), the
 * others are opened with hipIpcOpenMemHandle. Every rank must hold the same
 * number of populations. */
int pmaf_peer_connect(pmaf_planner *h, int32_t world, int32_t rank, const void *handles);
/* couple population `pop`'s trailing obstacle to the set-point of population
 * src_pop on rank src_rank (src_rank < 0: uncouple). init_pos [3] (may be
 * NULL) = the source's position the FIRST tick uses (only before the first
 * pmaf_tick after pmaf_peer_connect); without it the first tick waits for a
 * header that only a previous tick could have published. */
int pmaf_peer_couple(pmaf_planner *h, int32_t pop, int32_t src_rank, int32_t src_pop, double radius,
                     const double *init_pos);
/* every rank must have stopped ticking (barrier) before ANY rank disconnects or
 * destroys its handle: peers store into this rank's inbox */
int pmaf_peer_disconnect(pmaf_planner *h);
/* observability / tests: the newest header [world][P][8] and its sequence
 * number [world][P] (-1: none yet) in this rank's inbox; a small blocking copy */
int pmaf_peer_read(pmaf_planner *h, double *headers, double *seq);
/* per pmaf_tick since the last call (oldest first, at most max_n; clears the
 * record): wait_us = time the manager kernel waited for the coupled header
 * (what the control path pays for the coupling; ~0 when the ranks keep pace),
 * publish_us = its stores into the peers' inboxes incl. the system-scope fence
 * (device clock) */
int pmaf_get_peer_times_us(pmaf_planner *h, double *wait_us, double *publish_us, int32_t max_n, int32_t *n);
/* what the connection rests on: *fine_grained = 1 if this handle's inbox is fine-grained device memory (stores of
 * another GPU become visible to a running kernel), 0 if the runtime could only export plain device memory -- then
 * pmaf_peer_connect refuses peers on ANOTHER device (PMAF_ERR_DEVICE) and only same-device peers (several processes on
 * one GPU) can be connected. Either pointer may be NULL. */
int pmaf_peer_info(pmaf_planner *h, int32_t *fine_grained, int32_t *world);
/* hipGetDeviceCount (0 without a usable HIP device) */
int pmaf_device_count(void);

/* ---- checkpoint / resume (no reference equivalent: its state lives in RAM) ---- */
/* Serialise the complete planner state of a handle (agents' rotation vectors
 * and known flags, paths, real agent incl. its trajectory, best-agent copy,
 * obstacle tables, scoring parameters) into a caller buffer of at least
 * pmaf_state_size(h) bytes, and restore it into a handle created with the same
 * dimensions. After a restore the planner continues bit-identically. */
size_t pmaf_state_size(const pmaf_planner *h);
int pmaf_save_state(pmaf_planner *h, void *blob, size_t bytes);
int pmaf_load_state(pmaf_planner *h, const void *blob, size_t bytes);

/* ---- measurement ---- */
/* HIP-event timing of the rollout launches: 0 off, 1 every launch, n > 1 every n-th launch (the events ride on the
 * kernel's own dispatch packet, but a timed dispatch still costs 3-5 us of device time per tick -- tools/ticklat.py,
 * profiles/r4_tick_overhead.txt -- so a throughput measurement samples) */
int pmaf_set_profiling(pmaf_planner *h, int32_t enable);
/* rollout launches since the last pmaf_reset_kernel_stats, timed or not (pmaf_get_kernel_stats's `launches` counts the
 * timed ones while profiling is on) */
int pmaf_get_launch_count(pmaf_planner *h, int64_t *launches);
/* accumulated rollout-kernel time (ms), launches and agent-steps since the last reset_stats */
int pmaf_get_kernel_stats(pmaf_planner *h, double *rollout_ms, int64_t *launches,
                          int64_t *agent_steps);
int pmaf_reset_kernel_stats(pmaf_planner *h);
/* chosen lanes-per-agent and grid of the rollout kernel */
int pmaf_get_launch_config(pmaf_planner *h, int32_t *lanes_per_agent,
                           int32_t *n_blocks, int32_t *lds_bytes);
/* Wave-per-agent handles with 61..256 field obstacles: how many waves share an agent's rollout (csrc/pmaf_k_mw.hip:
 * one block of 2..4 waves per agent, <= 64 obstacles per wave, one LDS hand-off per step) and how many obstacles each
 * wave holds; waves_per_agent = 1: the one-wave kernels (2 / 4 obstacle slots per lane; always with
 * PMAF_FLAG_IEEE_SEQUENCES). Chosen at pmaf_create while
 * every wave of the launch gets a SIMD of its own; PMAF_MW=0 in the environment keeps the one-wave kernels, PMAF_MW=3|4
 * asks for more waves than the obstacle count needs (tests, timing). Results are bit-identical either way. */
int pmaf_get_waves_per_agent(pmaf_planner *h, int32_t *waves_per_agent, int32_t *obstacles_per_wave);
/* Whether the handle's rollout launches run the wave-per-agent kernel's PRIORITY-SLICING loop (k_rollout_w64_sliced): with
 * 1 025 ... 2 048 one-slot wave-per-agent rollouts in the handle two waves share a SIMD, the issue arbiter would serve the older
 * one first (the launch then lasts 1.64 x a lone wave's rollout), and the two trade issue priority in slices of the 100 MHz
 * wall clock instead (slice_ticks x 10 ns each, the younger wave holding `younger_of_8` of every eight) so that both finish
 * together: -4 ... -7 % per launch (profiles/r6_slice_sweep.txt). Scheduling only -- the arithmetic is the same instruction
 * sequence, results are bit-identical. No counterpart in the reference (the OS schedules its threads). */
int pmaf_get_priority_slices(pmaf_planner *h, int32_t *enabled, int32_t *slice_ticks, int32_t *younger_of_8);
/* The mapping rule as a pure function (no handle, no device): the lanes-per-agent mapping pmaf_create chooses for
 * n_populations x n_agents agents and n_field_obstacles circular-field obstacles (M, without the trailing repulsive one)
 * when pmaf_params.lanes_per_agent is 0, on a device with n_simds SIMDs (0 = MI355X's 1024). The reference has no
 * counterpart (it runs one std::thread per agent, B/src/cf_manager.cpp:118-123); this is the scheduling decision that
 * replaces it. 0 on invalid arguments. The rule is a table of measured launch times (csrc/pmaf_lpa_model.hpp,
 * profiles/r6_lpa_grid.txt); pmaf_estimate_rollout_us returns its estimate of the rollout kernel's duration in
 * microseconds for one mapping (lanes_per_agent in {64, 32, 16, 8}; horizon = steps per rollout) or a negative value
 * when the mapping is not offered for that obstacle count (a narrower mapping than the wave per agent holds at most two
 * obstacles per lane). Estimates, not promises: capacity planning (how many populations fit a control period) and the
 * tests that hold the rule to the measured grid (tests/test_lpa_model.py). */
int32_t pmaf_pick_lanes_per_agent(int32_t n_agents, int32_t n_populations, int32_t n_field_obstacles, int32_t n_simds);
double pmaf_estimate_rollout_us(int32_t lanes_per_agent, int32_t n_agents, int32_t n_populations, int32_t n_field_obstacles,
                                int32_t horizon, int32_t n_simds);

/* Measurement tooling (tools/slackprof): from now on the handle's rollout launches run `kernel_name` out of the code
 * object file at `code_object_path` (same arguments, grid and LDS as the built-in wave-per-agent kernel: the product
 * kernel's own assembly with delay instructions inserted); NULL path = back to the built-in kernels. Wave-per-agent
 * handles only. */
int pmaf_debug_external_rollout(pmaf_planner *h, const char *code_object_path, const char *kernel_name);
/* Fault injection for the tick's time limit (tests): while enabled, the manager kernel of pmaf_tick does not publish
 * its sequence number, so the host's wait can only end by the time limit (or by the stream running empty). */
int pmaf_debug_withhold_mailbox(pmaf_planner *h, int32_t enable);

/* Self-test of the device arithmetic the parity argument rests on: evaluates
 * op over n elements ON THE GPU (0: a/b, 1: sqrt(a), 2: the kernels' portable exp(a), 3: a*b,
 * 4: a+b; 5: the kernels' guarded sqrt, 6: guarded divide, 7 / 8: vector /
 * scalar through the guarded / the compiler's divide; 9 / 10: a / sqrt(b)
 * through the kernels' shared-reciprocal sequence / the compiler; 11 / 12: the
 * fixup-free a / b and a / sqrt(b) used where the divisor is a positive
 * normal; 13: the default policy's square root without its zero / infinity
 * select, for a positive finite a). Tests compare the results bitwise with
 * the host's IEEE results and with constructed hard-to-round operands
 * (tests/hard_rounding.py).
 * 14..17: the opt-in fast policy's operations, which carry an error bound
 * instead: 14: a / b through its refined reciprocal, 15: its sqrt(a), 16: the
 * reciprocal root y ~ 1 / sqrt(b) its norm sequence shares, 17: a / sqrt(b) as
 * the product a * y that replaces the division by a norm.
 * 18: the default policy's refined reciprocal of b by itself (a is ignored):
 * RN(1 / b); 19: the reciprocal of the double sqrt(b), taken from the root's own
 * iteration as the kernels' norms take it (a is ignored; b positive and
 * finite); 20: a / sqrt(b) through that reciprocal and the fixup-free
 * division. Compared bitwise like ops 5..13 (tests/test_rcp_bias_gpu.py). */
int pmaf_debug_math(int32_t op, int32_t n, const double *a, const double *b, double *out);

#ifdef __cplusplus
}
#endif
#endif /* PMAF_H */
