// pmaf_k_track.hip -- the repulsive track (include/pmaf.h "repulsive track"): k_rollout_w64_track, the one-slot
// wave-per-agent rollout whose trailing repulsive obstacle follows a per-step track instead of o + k v dt, and
// k_track_from_best, which copies a population's selected path into another population's track. A translation unit
// and an object of its own: the other units' code objects do not move with it.
//
// The step is rollout_w64_body of pmaf_rollout_w64_body.hpp, instantiated here -- and only here -- with TRACK = true.
// What TRACK adds to the loop that carries code for the repulsive obstacle (SENT == 1, the obstacle in lane 60): one
// 24-byte load from a wave-uniform address at the top of the step, for the step after it, and three selects behind the
// tail's O.p += O.v dt that put the point into lane 60. The loop without code for the obstacle (SENT == 0) is the same
// instantiation as in k_rollout_w64. track_reachable, which decides between the two for a track, is in that header too.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "pmaf_rollout_w64_body.hpp"
#include "pmaf_track.hpp"

using namespace pmaf;

template <bool DPPSUM, bool PLAIN>
__global__ __launch_bounds__(64) void k_rollout_w64_track(DevView D, CostParams CP, TrackArgs T) {
  constexpr int MATH = MATH_XACT;
  const int lane = threadIdx.x;
  const int pop = blockIdx.y;
  const int a = blockIdx.x;  // grid.x == N
  const int n_obs = D.n_obs, M = n_obs - 1;
  const double *src = D.obs_start + (size_t)pop * 7 * n_obs;
  const V3 p0 = mk(D.start_pos[pop * 3], D.start_pos[pop * 3 + 1], D.start_pos[pop * 3 + 2]);
  const PopConst C0 = D.C;
  // the population's track; a length of 0 (none attached, or the source population has no selection yet) leaves the
  // obstacle on its straight line: rollout_w64_dispatch's decision and the body's untracked path
  const int L = T.len[pop];
  const double *trk = T.track + (size_t)pop * T.max_len * 3;
  PMAF_BOUND(L >= 0 && L <= T.max_len);
  bool reach;
  if (L > 0) {
    reach = track_reachable(lane, p0, trk, (L < D.cap) ? L : D.cap, D.zsent_lt[pop], C0, D.cap);
  } else {
    const V3 sp = mk(src[M], src[n_obs + M], src[2 * n_obs + M]);
    const V3 sv = mk(src[3 * n_obs + M], src[4 * n_obs + M], src[5 * n_obs + M]);
    reach = sentinel_reachable(p0, sp, sv, D.zsent_lt[pop], C0, D.cap);
  }
  // (as in rollout_w64_dispatch: field obstacles at rest and the rel_vel rider's lane idle)
  const bool st = field_obstacles_at_rest(src, n_obs, M, lane, C0.dt) && (M <= 59 || !reach);
#define PMAF_BODY(T_) \
  if (st) { \
    if (!reach) rollout_w64_body<1, T_, MATH, 0, DPPSUM, PLAIN, true, false>(D, CP, lane, pop, a); \
    else rollout_w64_body<1, T_, MATH, 1, DPPSUM, PLAIN, true, false, true>(D, CP, lane, pop, a, trk, L); \
  } else if (!reach) rollout_w64_body<1, T_, MATH, 0, DPPSUM, PLAIN, false, false>(D, CP, lane, pop, a); \
  else rollout_w64_body<1, T_, MATH, 1, DPPSUM, PLAIN, false, false, true>(D, CP, lane, pop, a, trk, L)
  PMAF_W64_EACH_TYPE(D.types[a], PMAF_BODY)
#undef PMAF_BODY
}

// One block per population; a population that is not coupled leaves its track (an uploaded one) alone.
__global__ __launch_bounds__(64) void k_track_from_best(DevView D, CoupleArgs A) {
  const int pop = blockIdx.x;
  const int lane = threadIdx.x;
  const int q = A.src_pop[pop];
  if (q < 0 || q >= D.P) return;
  if (D.has_best[q] == 0) {
    if (lane == 0) A.len[pop] = 0;
    return;
  }
  int b = D.best_idx[q];
  b = (b < 0) ? 0 : ((b >= D.N) ? D.N - 1 : b);
  const size_t qa = (size_t)q * D.N + b;
  int n = D.n_points[qa];
  n = (n < 1) ? 1 : ((n > D.cap) ? D.cap : n);
  const int first = (A.shift < n - 1) ? A.shift : (n - 1);
  int len = n - first;   // == max(n - shift, 1)
  if (len > A.max_len) len = A.max_len;
  const double *src = A.paths + (qa * (size_t)D.cap + (size_t)first) * 3;
  double *dst = A.track + (size_t)pop * A.max_len * 3;
  for (int i = lane; i < 3 * len; i += 64) dst[i] = src[i];
  if (lane == 0) A.len[pop] = len;
}

bool pmaf_k_launch_w64_track(const DevView &D, const CostParams &cp, const TrackArgs &T, bool dppsum, bool plain, size_t lds,
                             hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  const dim3 g64((unsigned)D.N, (unsigned)D.P), block(64);
#define PMAF_L(K) hipExtLaunchKernelGGL(K, g64, block, (unsigned)lds, s, e0, e1, 0, D, cp, T)
  if (dppsum) { if (plain) PMAF_L((k_rollout_w64_track<true, true>)); else PMAF_L((k_rollout_w64_track<true, false>)); }
  else { if (plain) PMAF_L((k_rollout_w64_track<false, true>)); else PMAF_L((k_rollout_w64_track<false, false>)); }
#undef PMAF_L
  return true;
}

void pmaf_k_launch_track_from_best(const DevView &D, const CoupleArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_track_from_best, dim3((unsigned)D.P), dim3(64), 0, s, D, A);
}
