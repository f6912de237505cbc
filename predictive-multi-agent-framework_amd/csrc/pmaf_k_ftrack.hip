// pmaf_k_ftrack.hip -- the obstacle tracks (include/pmaf.h "obstacle tracks"): k_rollout_w64_ftrack, the one-slot
// wave-per-agent rollout whose M field obstacles follow per-step tracks (position and velocity) instead of o + k v dt,
// and whose trailing repulsive obstacle may follow a repulsive track as in k_rollout_w64_track. A translation unit and an
// object of its own (ftrack.o): the other units' code objects do not move with it.
//
// The step is rollout_w64_body of pmaf_rollout_w64_body.hpp, instantiated here -- and only here -- with FTRACK = true (and TRACK =
// true: one kernel serves field tracks, a repulsive track, or both, with empty lane masks for whatever is absent). What
// FTRACK adds to the loop: six 8-byte loads per lane at the top of the step, for the step after it -- lane i reads
// obstacle i's column of the point, the rows contiguous across the lanes -- and six selects behind the tail's
// O.p += O.v dt that put position and velocity into lanes 0 .. M-1. Lanes 60 .. 63 are never touched.
// The bodies that assume field obstacles at rest (STATICV) are not instantiated: a population with tracks moves whatever
// its live list says, and one without tracks in the same launch computes the same bits in the general body.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "pmaf_rollout_w64_body.hpp"
#include "pmaf_ftrack.hpp"

using namespace pmaf;

static_assert(PMAF_FTRACK_LANES == 64 && PMAF_FTRACK_POINT == 384, "rollout_w64_body's FTRACK loads assume [6][64] doubles per point");

template <bool DPPSUM, bool PLAIN>
__global__ __launch_bounds__(64) void k_rollout_w64_ftrack(DevView D, CostParams CP, TrackArgs T, FTrackArgs F) {
  constexpr int MATH = MATH_XACT;
  const int lane = threadIdx.x;
  const int pop = blockIdx.y;
  const int a = blockIdx.x;  // grid.x == N
  const int n_obs = D.n_obs, M = n_obs - 1;
  const double *src = D.obs_start + (size_t)pop * 7 * n_obs;
  const V3 p0 = mk(D.start_pos[pop * 3], D.start_pos[pop * 3 + 1], D.start_pos[pop * 3 + 2]);
  const PopConst C0 = D.C;
  // the trailing obstacle: as in k_rollout_w64_track
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
  // the field obstacles: the population's tracks, 0 points = none (the body's untracked path; the loads still touch point 0)
  const int FL = F.len[pop];
  const int first = F.first[pop];
  const double *ftrk = F.pts + (size_t)pop * F.max_len * PMAF_FTRACK_POINT;
  PMAF_BOUND(M <= 60 && FL >= 0 && FL <= F.max_len && first >= 0);
#define PMAF_BODY(T_) \
  if (!reach) rollout_w64_body<1, T_, MATH, 0, DPPSUM, PLAIN, false, false, true, true>(D, CP, lane, pop, a, trk, L, ftrk, FL, first); \
  else rollout_w64_body<1, T_, MATH, 1, DPPSUM, PLAIN, false, false, true, true>(D, CP, lane, pop, a, trk, L, ftrk, FL, first)
  PMAF_W64_EACH_TYPE(D.types[a], PMAF_BODY)
#undef PMAF_BODY
}

bool pmaf_k_launch_w64_ftrack(const DevView &D, const CostParams &cp, const TrackArgs &T, const FTrackArgs &F, bool dppsum,
                              bool plain, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  const dim3 g64((unsigned)D.N, (unsigned)D.P), block(64);
#define PMAF_L(K) hipExtLaunchKernelGGL(K, g64, block, (unsigned)lds, s, e0, e1, 0, D, cp, T, F)
  if (dppsum) { if (plain) PMAF_L((k_rollout_w64_ftrack<true, true>)); else PMAF_L((k_rollout_w64_ftrack<true, false>)); }
  else { if (plain) PMAF_L((k_rollout_w64_ftrack<false, true>)); else PMAF_L((k_rollout_w64_ftrack<false, false>)); }
#undef PMAF_L
  return true;
}
