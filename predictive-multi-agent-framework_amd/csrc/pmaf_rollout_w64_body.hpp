// pmaf_rollout_w64_body.hpp -- the step of the wave-per-agent rollout: rollout_w64_body, its per-heuristic dispatch and
// what the kernels that instantiate it share. Device code only (hipcc); included by pmaf_k_w64.hip (k_rollout_w64,
// k_rollout_w64_sliced), pmaf_k_track.hip (k_rollout_w64_track) and pmaf_k_ftrack.hip (k_rollout_w64_ftrack).
// The units share this TEXT and nothing else: in the rollout kernels a helper function or a generic lambda between the
// kernel and the body moves the step loop's schedule (NOTES.md 1), so what varies per kernel is passed as a macro
// (PMAF_W64_EACH_TYPE) and the functions below live at global scope like the kernels that call them.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_rollout_w64.hpp"
#include "pmaf_rollout_grp.hpp"

using namespace pmaf;

// the heuristic dispatch: BODY(T) for the wave's heuristic T (uniform per wave), written once for every kernel above
#define PMAF_W64_EACH_TYPE(type, BODY) \
  switch (type) { \
    case T_GOAL: BODY(T_GOAL); break; \
    case T_OBST: BODY(T_OBST); break; \
    case T_GOALOBST: BODY(T_GOALOBST); break; \
    case T_VEL: BODY(T_VEL); break; \
    case T_RANDOM: BODY(T_RANDOM); break; \
    case T_HAD: BODY(T_HAD); break; \
    default: break; \
  }

// sentinel_reachable (pmaf_rollout_w64.hpp) for a track: can ANY point the rollout may read -- y_0 ... y_{min(L, cap) - 1},
// the held last one included -- come into repelForce's range? The agent is never farther than steps * per_step from its
// start (|a| <= 13, |v| <= vel_max, both clamped), whatever step a point belongs to, so a point farther than
// range + reach from the start is out of range at every step. Same margins as sentinel_reachable; lanes stride over the
// points. Conservative only: the loop it selects computes the same bits either way.
// (here and not in pmaf_track.hpp: the host units include that one)
__device__ __forceinline__ bool track_reachable(int lane, V3 p0, const double *trk, int n_pts, double zsent_lt,
                                                const PopConst &C, int steps) {
  const double adt = fabs(C.dt);
  const double per_step = 6.5 * adt * adt + fabs(C.vel_max) * adt;
  const double reach = (double)steps * per_step * 1.001 + 1e-9;
  const double range = __builtin_sqrt(zsent_lt) * 1.001;
  bool any = false;
  for (int j = lane; j < n_pts; j += 64) {
    const V3 y = mk(trk[3 * j], trk[3 * j + 1], trk[3 * j + 2]);
    any = any || !(norm(p0 - y) > range + reach);   // NaN anywhere: keep testing
  }
  return wave_any(any);
}

// ---------------------------------------------------------------------------
// k_rollout_w64<TILES>: one wave64 per agent (see pmaf_rollout_w64.hpp)
// ---------------------------------------------------------------------------
// the step loop, specialised on the agent's heuristic so the per-step code
// carries no type dispatch (the type is uniform per wave)
// SENT: 0 = the repulsive obstacle cannot come into range during this rollout (decided by the caller, one-slot kernel
// only: the step loop then has no block for it), 1 = it can, 2 = decide here at run time (the other kernels)
// PLAIN: every agent of the launch has k_attr != 0 and the agents have unit mass (the reference's defaults and every
// shipped task file; decided by the host at pmaf_create): the step then carries neither the `k_attr != 0` select nor the
// division by the mass -- for a lone wave every instruction is an issue slot
// (ONE LDS copy of exp's data per block: a __shared__ array declared inside rollout_w64_body would be one array per
// instantiation of the body -- six heuristics = 12.4 KB of static LDS per one-wave block, and 2048+ agents x 129 obstacles
// no longer fit eight blocks to a CU: +45 % on those launches, found by tools/regime.py's sweep)
__device__ __forceinline__ double *w64_exp_lds() {
  __shared__ double s_expk[EXPK_N];
  return s_expk;
}
template <int TILES>
__device__ __forceinline__ auto w64_exp_consts(int lane) {
  if constexpr (TILES >= 2) {
    double *tab = w64_exp_lds();
    exp_consts_to_lds(tab, lane);
    wave_lds_fence();
    return exp_consts_from_lds(tab);
  } else {
    return exp_consts_in_vgprs();
  }
}
// STATICV (one slot per lane): every field obstacle of the population is at rest (+0.0 velocities, no -0.0 coordinate,
// 0 <= dt < inf: field_obstacles_at_rest) and the lane the rel_vel rider needs is idle -- decided per block by the
// kernel (pmaf_rollout_w64.hpp, NVL)
// SLICE (round 6): launches of MORE waves than the device has SIMDs -- 1 025 ... 2 048 agents on this kernel: two waves on
// half or all of the SIMDs. The issue arbiter serves the older wave first, absolutely: the first n_simds waves run at their
// stand-alone speed T, the others on the slots left over (0.42 of a wave's rate) and then alone, 1.58 T in all (232 -> 375 us
// at 2 048 agents x 32 obstacles, profiles/r6_lpa_band.txt). With SLICE the two waves of a SIMD trade issue priority in
// slices of the wall clock (the group kernel's scheme, pmaf_k_grp.hip) so that both finish together at 2 T / 1.42.
// A template parameter, not a run-time flag: the one-wave-per-SIMD launches (C1, C2, C4) keep their step loop untouched.
// TRACK (pmaf_k_track.hip only: every kernel of pmaf_k_w64.hip leaves it false): the repulsive obstacle follows
// the population's repulsive track (include/pmaf.h "repulsive track") -- trk = its points [trk_len][3], trk_len == 0: no
// track, the straight line as ever. One-slot kernel only; the loop without code for the obstacle (SENT == 0) never reads it.
// FTRACK (pmaf_k_ftrack.hip only, together with TRACK): the field obstacles follow the population's obstacle tracks
// (include/pmaf.h "obstacle tracks") -- ftrk = its points [ftrk_len][6][64] (position and velocity, one obstacle per lane:
// the six loads of a step are contiguous across the lanes), ftrk_first = the offset; ftrk_len == 0: none, the straight
// lines as ever. One-slot kernel, never the STATICV bodies: a tracked obstacle moves whatever the live list says.
template <int TILES, int TYPE, int MATH, int SENT = 2, bool DPPSUM = false, bool PLAIN = false, bool STATICV = false, bool SLICE = false,
          bool TRACK = false, bool FTRACK = false>
__device__ __forceinline__ void rollout_w64_body(const DevView &D, const CostParams &CP, const int lane,
                                                 const int pop, const int a, const double *trk = nullptr,
                                                 const int trk_len = 0, const double *ftrk = nullptr,
                                                 const int ftrk_len = 0, const int ftrk_first = 0) {
  static_assert(!TRACK || (TILES == 1 && SENT != 2), "the repulsive track rides in lane 60 of the one-slot kernel");
  static_assert(!FTRACK || (TILES == 1 && SENT != 2 && !STATICV && TRACK), "the obstacle tracks ride in lanes 0 .. M-1 of the one-slot kernel");
  extern __shared__ double smem[];
  const unsigned long long t_begin = wall_clock64();
  const int n_obs = D.n_obs;
  const int M = n_obs - 1;
  // Loop-invariant wave-uniform doubles (population constants, goal, gains, the exp() coefficients) are pinned
  // into VGPRs: left to itself the compiler keeps them in the 100-odd SGPRs, runs out, and pays for the
  // spills (v_writelane / v_readlane) in the step loop -- 163 spilled SGPRs before, C2 360 -> 344 us with this.
  PopConst C = D.C;
  { double *f = reinterpret_cast<double *>(&C);
    for (int i = 0; i < (int)(sizeof(PopConst) / sizeof(double)); i++) asm volatile("" : "+v"(f[i])); }
  // (two and four slots per lane have no VGPRs to spare for the exp coefficients: measured)
  // portable_exp's twelve constants: pinned in VGPRs in the one-slot kernel; the multi-slot kernels sit at the
  // 256-VGPR ceiling and fetch them from an LDS table right where the chain uses them (one box, C3: 1151 -> 1128 us
  // against literals / SGPRs; the one-slot kernel the other way round, C2 243 against 264 us: profiles/r3_ab_exp.txt)
  const auto EK = w64_exp_consts<TILES>(lane);
  const size_t pa = (size_t)pop * D.N + a;
  const double *src = D.obs_start + (size_t)pop * 7 * n_obs;
  const int32_t *ks = D.known_start + (size_t)pop * n_obs;
  double *rot_g = D.rot + pa * 3 * n_obs;
  const double *rnd_g = D.rnd + pa * 3 * n_obs;

  LaneObstacles<TILES> O;
  unsigned known_bits = 0u;
  // closest-other table (below): the multi-slot kernels' Obstacle / GoalObstacle bodies only -- with one slot per lane
  // the search is one sqrt chain + two reductions, the GoalObstacle agent does not bound the C2 launch without it, and
  // the short C1 rollout would pay for the table's loads in its prologue (measured: profiles/r3_ab_session3.txt)
  constexpr bool USES_CLOSEST = TILES >= 2 && (TYPE == T_OBST || TYPE == T_GOALOBST);
#pragma unroll
  for (int t = 0; t < TILES; t++) {
    int i = t * 64 + lane;
    bool valid = i < M;
    int ii = valid ? i : 0;
    O.p[t] = mk(src[ii], src[n_obs + ii], src[2 * n_obs + ii]);
    O.v[t] = mk(src[3 * n_obs + ii], src[4 * n_obs + ii], src[5 * n_obs + ii]);
    O.r[t] = src[6 * n_obs + ii];
    O.rx[t] = rot_g[ii]; O.ry[t] = rot_g[n_obs + ii]; O.rz[t] = rot_g[2 * n_obs + ii];
    if (TYPE == T_RANDOM) { O.qx[t] = rnd_g[ii]; O.qy[t] = rnd_g[n_obs + ii]; O.qz[t] = rnd_g[2 * n_obs + ii]; }
    else { O.qx[t] = 0.0; O.qy[t] = 0.0; O.qz[t] = 0.0; }
    if (valid && ks[ii]) known_bits |= (1u << t);
  }
  // trailing repulsive obstacle, wave-uniform
  V3 sent_p = mk(src[M], src[n_obs + M], src[2 * n_obs + M]);
  const V3 sent_v = mk(src[3 * n_obs + M], src[4 * n_obs + M], src[5 * n_obs + M]);
  const double sent_r = src[6 * n_obs + M];
  // the track's first point is the obstacle of step 0 (y_0 in place of o_M); the pointer lives in a VGPR pair so that
  // the per-step fetch below is ONE vector load from a wave-uniform address, like the path store, and not a scalar
  // load on the LDS instructions' counter -- and it is a GLOBAL pointer (the pin alone would leave a generic one: flat
  // loads, which count on that counter as well)
  typedef const __attribute__((address_space(1))) double *gptr;
  gptr trk_v = (gptr)trk;
  const int trk_last = (trk_len > 0) ? (trk_len - 1) : 0;
  const lmask trk_m = (TRACK && SENT == 1 && trk_len > 0) ? (1ull << 60) : 0ull;
  if (TRACK && SENT == 1) {
    asm volatile("" : "+v"(trk_v));
    if (trk_len > 0) sent_p = mk(trk_v[0], trk_v[1], trk_v[2]);
  }
  // obstacle tracks: lane i < M takes obstacle i's position and velocity of point min(first, L-1) for step 0. The lane's
  // pointer (its column of the [6][64] block of a point) is a global one in a VGPR pair like trk_v: six vector loads
  // per step at immediate offsets, on vmcnt. Lanes >= M load their zero-filled columns and never use them.
  gptr ftrk_v = (gptr)ftrk + lane;
  const int ftrk_last = (ftrk_len > 0) ? (ftrk_len - 1) : 0;
  const int ftrk_at = (ftrk_first < ftrk_last) ? ftrk_first : ftrk_last;   // point of step 0; step k: min(ftrk_at + k, last)
  const lmask ftrk_m = (FTRACK && ftrk_len > 0) ? ((1ull << M) - 1ull) : 0ull;
  if (FTRACK) {
    asm volatile("" : "+v"(ftrk_v));
    const gptr fp = ftrk_v + (size_t)ftrk_at * 384;
    const bool fl = PMAF_LANE(ftrk_m);
    O.p[0].x = fl ? fp[0] : O.p[0].x; O.p[0].y = fl ? fp[64] : O.p[0].y; O.p[0].z = fl ? fp[128] : O.p[0].z;
    O.v[0].x = fl ? fp[192] : O.v[0].x; O.v[0].y = fl ? fp[256] : O.v[0].y; O.v[0].z = fl ? fp[320] : O.v[0].z;
  }

  V3 goal = mk(D.goal[pop * 3], D.goal[pop * 3 + 1], D.goal[pop * 3 + 2]);
  V3 init_pos = mk(D.agent_init_pos[pop * 3], D.agent_init_pos[pop * 3 + 1], D.agent_init_pos[pop * 3 + 2]);
  asm volatile("" : "+v"(goal.x), "+v"(goal.y), "+v"(goal.z), "+v"(init_pos.x), "+v"(init_pos.y), "+v"(init_pos.z));
  V3 p = mk(D.start_pos[pop * 3], D.start_pos[pop * 3 + 1], D.start_pos[pop * 3 + 2]);
  V3 v = mk(D.start_vel[pop * 3], D.start_vel[pop * 3 + 1], D.start_vel[pop * 3 + 2]);
  double k_attr = D.k_attr[pa], k_circ = D.k_circ[pa], k_repel = D.k_repel[pa], k_damp = D.k_damp[pa];
  asm volatile("" : "+v"(k_attr), "+v"(k_circ), "+v"(k_repel), "+v"(k_damp));
  double *path = D.paths + pa * (size_t)D.cap * 3;

  // LDS list of the step's non-zero circular-field terms (after the obstacle table)
  int clist_off = 7 * n_obs + (n_obs + 1) / 2;
  clist_off += clist_off & 1;
  double *clist = smem + clist_off;

  double lane_min = C.shell;  // per-lane running min_obs_dist_, reduced once after the loop
  int n = 1;
  bool ran = false;
  if (lane == 0) { path[0] = p.x; path[1] = p.y; path[2] = p.z; }

  // Everything the next step needs from the new state -- goal distance (loop
  // guard / gate), goal direction, squared speed, squared start distance and
  // attractorForce's velocity error (B/src/cf_agent.cpp:188-192) -- is computed
  // at the END of the step in one basic block with the velocity clamp and the
  // path-length norm: five independent sqrt / divide chains that the in-order
  // issue of a lone wave can only overlap inside one block.
  typedef Mth<MATH> MT;
  V3 g = goal - p;
  double dg = MT::norm(g);
  double zv = sqn(v);
  double z_init = sqn(p - init_pos);
  V3 gn = (dg > 0.0) ? MT::div3(g, dg) : g;  // goal_vec.normalized()
  // One slot per lane (M <= 60; the host sends 61..64 obstacles to the split / two-slot kernels): the sweep's |ro| /
  // ro.normalized() of the NEXT step are computed at the end of this step, and the lanes that have no obstacle carry
  // the tail's other norms through the same instructions -- lane 63 the goal (distance and direction), lane 62 the
  // speed clamp, lane 61 attractorForce's speed limit -- instead of three more sqrt / reciprocal / divide sequences.
  constexpr bool PRE = (TILES == 1);
  double s_pre = 0.0;
  V3 ron_pre = mk(0.0, 0.0, 0.0);
  // attractorForce's desired velocity (k_attr / k_damp) * g rides in lane 61 as `other * lane_scale`: the lane holds the
  // goal like lane 63 (one-slot kernel; the others use g directly) and lane_scale is the gain ratio there, 1.0 in every
  // other lane (x * 1.0 == x): three multiplies instead of three 64-bit selects per step
  double lane_scale = (lane == 61) ? (k_attr / k_damp) : 1.0;
  asm volatile("" : "+v"(lane_scale));
  if (PRE) {
    // (velocity -0.0 for dt >= 0: p + (-0.0) dt leaves EVERY p as it is, a -0.0 goal coordinate included -- with +0.0
    // it would turn into +0.0, and the goal direction read back from lane 63 also feeds the latch, calc_rot_vec_pre)
    const double nz = (C.dt < 0.0) ? 0.0 : -0.0;
    if (lane == 63 || lane == 61) { O.p[0] = goal; O.v[0] = mk(nz, nz, nz); }
    // Round 4 (last session): the loop that carries code for the repulsive obstacle keeps that obstacle in lane 60 like a
    // field obstacle (advanced with the others by predictObstacles' p + v dt), so that |p - sent_pos| and the direction
    // to it -- repelForce's square root, reciprocal and three divisions -- ride in the tail's ONE sequence like the goal
    // and the two speed limits (the one-slot kernel therefore takes at most 60 field obstacles; the host sends 61..64
    // to the other kernels). C4, where the obstacle is the other arm: 280.0 -> 270.5 us per launch
    // (profiles/r4_ab_w64.txt item 8).
    if (SENT == 1 && lane == 60) { O.p[0] = sent_p; O.v[0] = sent_v; }
    MT::norm_unit(O.p[0] - p, s_pre, ron_pre);
  }
  constexpr bool SRIDE = PRE && SENT == 1;
  V3 verr = attractor_velocity_error<MATH>(v, g, C, k_attr, k_damp);
  const double zsent_lt = D.zsent_lt[pop];
  const bool sent_reachable = (SENT == 2) ? sentinel_reachable(p, sent_p, sent_v, zsent_lt, C, D.cap) : (SENT == 1);
  bool moving = false;  // any field obstacle with a non-zero (or NaN) velocity component
#pragma unroll
  for (int t = 0; t < TILES; t++) moving = moving || !(O.v[t].x == 0.0 && O.v[t].y == 0.0 && O.v[t].z == 0.0);
  moving = wave_any(moving);
  bool advance = true;
  // Closest-other table (Obstacle / GoalObstacle heuristics only; DevView::closest_idx): valid when k_manager computed
  // it for this rollout's start obstacles and they are at rest. The wave keeps its copy in the obstacle-table area of
  // the LDS layout, which this kernel does not use otherwise (its obstacles live in registers).
  const int32_t *cidx = nullptr;
  if (USES_CLOSEST) {
    if (!moving && D.closest_ok[pop] == 1) {   // wave-uniform
      int32_t *s_cidx = reinterpret_cast<int32_t *>(smem);
      const int32_t *ci = D.closest_idx + (size_t)pop * n_obs;
#pragma unroll
      for (int t = 0; t < TILES; t++) {
        const int i = t * 64 + lane;
        if (i < M) s_cidx[i] = ci[i];
      }
      wave_lds_fence();
      cidx = s_cidx;
    }
  }
  V3 repel = mk(0.0, 0.0, 0.0);  // repelForce of the coming step (depends on the step's start state only)
  const double inv_shell = (SENT == 0) ? 0.0 : 1.0 / C.shell;   // (sentinel_repel_m)
  if (sent_reachable) repel = sentinel_repel_m<MATH>(p, C, k_repel, sent_p, sent_r, zsent_lt, inv_shell);
  SecTimers ST;
#ifdef PMAF_SECTION_TIMERS
  ST.start();
#endif
  const bool younger = SLICE && ((((unsigned)blockIdx.y * gridDim.x + blockIdx.x) / (unsigned)D.n_simds) & 1u) != 0u;
  const unsigned slice_log2 = (unsigned)D.prio_slice_log2, younger_of_8 = (unsigned)D.prio_younger_of_8;
  // Two step loops over ONE text (pmaf_rollout_w64_step.hpp). The short loop is the step as it always was: its ordered
  // sum adds one chunk of 16 terms in the block of the scaling chain and leaves that block for a rare loop when the list
  // is longer. Long lists come in a few long runs per rollout (profiles/c2_long_loop.md), so the first step that meets
  // one (circ_and_scale_w64 zeroes short_cap in that rare loop: nothing on the common path) ends the short loop through
  // its guard -- the compare with the capacity it always had -- and the rollout goes on in the long loop, whose sum adds
  // the second chunk in the block as well (LONG). The long loop is never left: a short list costs it sixteen accumulates
  // of +0.0 and six instructions round them, 22 issue slots of ~460 per step, and the agent that bounds a launch has few.
  // Every other instantiation keeps its one loop, with the call as it was (PMAF_STEP_FLAG: the call's last argument).
  if constexpr (TILES == 1 && DPPSUM) {
    int short_cap = D.cap;
    while ((dg > 0.1) && (n < short_cap)) {  // wave-uniform guard, B/src/cf_agent.cpp:310-311
#define PMAF_STEP_LONG false
#define PMAF_STEP_FLAG , &short_cap
#include "pmaf_rollout_w64_step.hpp"
#undef PMAF_STEP_LONG
    }
    while ((dg > 0.1) && (n < D.cap)) {
#define PMAF_STEP_LONG true
#include "pmaf_rollout_w64_step.hpp"
#undef PMAF_STEP_LONG
#undef PMAF_STEP_FLAG
    }
  } else {
    while ((dg > 0.1) && (n < D.cap)) {  // wave-uniform guard, B/src/cf_agent.cpp:310-311
#define PMAF_STEP_LONG false
#define PMAF_STEP_FLAG
#include "pmaf_rollout_w64_step.hpp"
#undef PMAF_STEP_LONG
#undef PMAF_STEP_FLAG
    }
  }
  if (SLICE) __builtin_amdgcn_s_setprio(0);
#ifdef PMAF_SECTION_TIMERS
  if (lane == 0 && pop == 0 && a < 7)
    printf("agent %d type %d steps %d | verr+gate %llu sweep %llu scale %llu circ %llu sum %llu (skip) %llu finish %llu tail %llu | "
           "in-shell steps %llu terms %llu\n", a, TYPE, n - 1, ST.acc[0], ST.acc[1], ST.acc[2], ST.acc[3], ST.acc[4],
           ST.acc[5], ST.acc[6], ST.acc[7], ST.cnt[0], ST.cnt[1]);
#endif

  double cost_ws, path_len;
#ifdef PMAF_SECTION_TIMERS
  const unsigned long long t_loop_end = wall_clock64();
#endif
  path_cost_terms_w64<MATH>(lane, path, n, CP.ws, CP.k_workspace, clist, cost_ws, path_len);
#ifdef PMAF_SECTION_TIMERS
  if (lane == 0 && pop == 0 && a < 7)
    printf("agent %d: loop %llu0 ns, path-cost pass %llu0 ns (%d points)\n", a, t_loop_end - t_begin, wall_clock64() - t_loop_end, n);
#endif

  const double min_obs = wave_min64(lane_min);
  int32_t *ko = D.known_out + pa * n_obs;
#pragma unroll
  for (int t = 0; t < TILES; t++) {
    int i = t * 64 + lane;
    if (i < M) ko[i] = (int32_t)((known_bits >> t) & 1u);
  }
  if (lane == 0) {
    ko[M] = ks[M];
    D.n_points[pa] = n;
    D.agent_vel[pa * 3] = v.x; D.agent_vel[pa * 3 + 1] = v.y; D.agent_vel[pa * 3 + 2] = v.z;
    D.min_obs[pa] = min_obs;
    D.cost_ws[pa] = cost_ws;
    D.path_len[pa] = path_len;
    D.goal_dist[pa] = dg;
    if (ran) D.reached[pa] = dg < 0.100001;  // B/src/cf_agent.cpp:330-337
    atomicAdd(D.step_counter, (unsigned long long)(n - 1));
    D.pred_ticks[pa] = wall_clock64() - t_begin;
  }
}

template <int TILES, int MATH, bool DPPSUM, bool PLAIN, bool SLICE>
__device__ __forceinline__ void rollout_w64_dispatch(const DevView &D, const CostParams &CP) {
  const int lane = threadIdx.x;
  const int pop = blockIdx.y;
  const int a = blockIdx.x;  // grid.x == N
  if (TILES == 1) {
    // one slot per lane: the repulsive obstacle's reachability (per rollout, see sentinel_reachable) picks a loop
    // without any code for it -- in the shipped scenes it sits 170 m away
    const int n_obs = D.n_obs, M = n_obs - 1;
    const double *src = D.obs_start + (size_t)pop * 7 * n_obs;
    const V3 sp = mk(src[M], src[n_obs + M], src[2 * n_obs + M]);
    const V3 sv = mk(src[3 * n_obs + M], src[4 * n_obs + M], src[5 * n_obs + M]);
    const V3 p0 = mk(D.start_pos[pop * 3], D.start_pos[pop * 3 + 1], D.start_pos[pop * 3 + 2]);
    const PopConst C0 = D.C;
    const bool reach = sentinel_reachable(p0, sp, sv, D.zsent_lt[pop], C0, D.cap);
    // field obstacles at rest (field_obstacles_at_rest: +0.0 velocities, no -0.0 coordinate, 0 <= dt < inf) and the
    // rider's lane idle (lane 60; 59 when lane 60 holds the repulsive obstacle): the loops with one normalisation
    // sequence less per step and, without the repulsive obstacle, no obstacle advance
    const bool st = field_obstacles_at_rest(src, n_obs, M, lane, C0.dt) && (M <= 59 || !reach);
#define PMAF_BODY(T) \
    if (st) { \
      if (!reach) rollout_w64_body<TILES, T, MATH, 0, DPPSUM, PLAIN, true, SLICE>(D, CP, lane, pop, a); \
      else rollout_w64_body<TILES, T, MATH, 1, DPPSUM, PLAIN, true, SLICE>(D, CP, lane, pop, a); \
    } else if (!reach) rollout_w64_body<TILES, T, MATH, 0, DPPSUM, PLAIN, false, SLICE>(D, CP, lane, pop, a); \
    else rollout_w64_body<TILES, T, MATH, 1, DPPSUM, PLAIN, false, SLICE>(D, CP, lane, pop, a)
    PMAF_W64_EACH_TYPE(D.types[a], PMAF_BODY)
#undef PMAF_BODY
    return;
  }
#define PMAF_BODY(T) rollout_w64_body<TILES, T, MATH, 2, DPPSUM, PLAIN>(D, CP, lane, pop, a)
  PMAF_W64_EACH_TYPE(D.types[a], PMAF_BODY)
#undef PMAF_BODY
}
