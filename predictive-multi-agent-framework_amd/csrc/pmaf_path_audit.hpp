// pmaf_path_audit.hpp -- kernels of pmaf_evaluate_paths / pmaf_evaluate_path (include/pmaf.h): the handle's CURRENT
// predicted paths audited against the caller's live obstacle list. The reference declares
// CfManager::evaluatePath(const std::vector<Obstacle> &) (B/include/bimanual_planning_ros/cf_manager.h:130) and never
// defines it; evaluateAgents ignores its obstacle list (B/src/cf_manager.cpp:293-356) and scores min_obs_dist_, which
// the rollout recorded against the obstacle copies of the previous reset (B/src/cf_agent.cpp:83-88). Included by
// pmaf_k_misc.hip (no translation unit of its own).
//
// Semantics (the host-side contract is in include/pmaf.h): for path point x_k of agent (p, a), k < n_points, and
// obstacle j of the list, the last (repulsive) one included,
//   o_j^0 = the caller's position, o_j^{k+1} = o_j^k + v_j * dt   (one multiply, one add per component, each rounded:
//                                                                  CfAgent::predictObstacles, B/src/cf_agent.cpp:270-276)
//   c(k, j) = norm(x_k - o_j^k) - (rad + r_j)                     (evalObstacleDistance, B/src/cf_agent.cpp:150-151;
//                                                                  no floor, no cap)
// clearance = min c by strict `<` from +inf (a NaN pair never wins), (step, obstacle) its argmin with ties to the
// smallest k, then the smallest j; first_violation = the smallest k with c(k, j) < margin for some j, else n_points;
// per_obstacle[j] = min over k of c(k, j).
//
// k_audit_track   one thread per (population, obstacle) walks k = 0 .. cap-1 and writes track[p][k][3][n_obs]: the
//                 track is a dependent chain of cap additions per obstacle and the same for every agent of the
//                 population, so it is built once per call (P * n_obs chains) instead of once per agent.
// k_path_audit    one block of four waves per (agent, population). The 64 lanes of a wave form 64 / G rows of
//                 G = min(64, 2^ceil(log2 n_obs)) lanes: lane (row, col) evaluates path point k = (wave * rows + row),
//                 stepping by 4 * rows, against obstacle j = tile * G + col; populations of more than 64 obstacles take
//                 one pass over the path per tile of 64. Why this shape:
//                  - a lane's obstacle index is fixed during a pass, so the per-obstacle minimum is ONE register per
//                    lane -- no per-obstacle array in LDS (n_obs is unbounded; static LDS here is 2 KB) and no
//                    indexed private array (no scratch);
//                  - the lanes of a row read G consecutive doubles of a track row and the rows of a wave consecutive
//                    track rows (coalesced); the path point is shared by a row (one cache line per wave and component);
//                  - with few obstacles the rows fill the wave with path points instead of idling 64 - n_obs lanes
//                    (n_obs = 2: 32 points per wave and pass).
//                 Every pair is independent: ~13 FP64 operations plus the correctly rounded square root; there is no
//                 chain as in the rollout, so the kernel relies on occupancy (small register footprint, 8 waves per
//                 SIMD) rather than on instruction-level parallelism. The track is re-read by every block of a population
//                 (P * N * n * n_obs * 24 bytes through L2); it is not staged in LDS because a block uses every element
//                 exactly once.
//                 Reductions are minima of doubles and integers only -- exact, associative and commutative for the
//                 values that can win (NaN never enters a running minimum) -- so the result does not depend on the
//                 order: lexicographic (c, k * n_obs + j) and the first violating k by __shfl_xor butterflies inside a
//                 wave, then through LDS across the four waves; per-obstacle minima by a butterfly over the rows (lane
//                 offsets >= G), then LDS across the waves. No atomics: results are bit-deterministic.
#pragma once
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"

namespace pmaf {

#define PMAF_AUDIT_WAVES 4

__global__ void k_audit_track(int P, int n_obs, int cap, double dt, const double *obs /*[P][7][n_obs]*/,
                              double *track /*[P][cap][3][n_obs]*/) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P * n_obs) return;
  const int pop = idx / n_obs, j = idx - pop * n_obs;
  const double *o = obs + (size_t)pop * 7 * n_obs;
  V3 q = mk(o[j], o[n_obs + j], o[2 * n_obs + j]);
  const V3 v = mk(o[3 * n_obs + j], o[4 * n_obs + j], o[5 * n_obs + j]);
  double *t = track + (size_t)pop * cap * 3 * n_obs + j;
  for (int k = 0; k < cap; k++) {
    t[0] = q.x; t[n_obs] = q.y; t[2 * (size_t)n_obs] = q.z;
    t += 3 * (size_t)n_obs;
    // predictObstacles, B/src/cf_agent.cpp:270-276
    q.x = q.x + v.x * dt;
    q.y = q.y + v.y * dt;
    q.z = q.z + v.z * dt;
  }
}

__global__ __launch_bounds__(64 * PMAF_AUDIT_WAVES) void k_path_audit(DevView D, AuditArgs A) {
  __shared__ double s_c[PMAF_AUDIT_WAVES];
  __shared__ int s_i[PMAF_AUDIT_WAVES], s_v[PMAF_AUDIT_WAVES];
  __shared__ double s_po[PMAF_AUDIT_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pop = blockIdx.y;
  const int n_obs = D.n_obs;
  // pmaf_evaluate_path: the selected agent only (best_id is 1-based; the host has checked that a selection exists)
  const int a = A.only_best ? D.best_id[pop] - 1 : (int)blockIdx.x;
  PMAF_BOUND(a >= 0 && a < D.N);
  const size_t pa = (size_t)pop * D.N + a;
  const size_t out = A.only_best ? (size_t)pop : pa;
  int n = D.n_points[pa];
  PMAF_BOUND(n >= 0 && n <= D.cap);
  n = n < D.cap ? n : D.cap;
  const double *path = D.paths + pa * (size_t)D.cap * 3;
  const double *trk = A.track + (size_t)pop * D.cap * 3 * n_obs;
  const double *rad_o = A.obs + (size_t)pop * 7 * n_obs + 6 * (size_t)n_obs;
  const int G = 1 << A.group_log2, rows = 64 >> A.group_log2;
  const int row = lane >> A.group_log2, col = lane & (G - 1);
  const double inf = __builtin_huge_val();

  double best_c = inf;
  int best_i = 0x7fffffff, viol = 0x7fffffff;
  for (int j0 = 0; j0 < n_obs; j0 += G) {   // one pass over the path per obstacle tile (block-uniform trip count)
    const int j = j0 + col;
    const bool jv = j < n_obs;
    const int jc = jv ? j : 0;
    const double rr = D.C.rad + rad_o[jc];
    double pmin = inf;
    for (int k = wave * rows + row; k < n; k += PMAF_AUDIT_WAVES * rows) {
      const V3 x = mk(path[k * 3], path[k * 3 + 1], path[k * 3 + 2]);
      const double *t = trk + (size_t)k * 3 * n_obs + jc;
      const V3 o = mk(t[0], t[n_obs], t[2 * (size_t)n_obs]);
      const double c = norm(x - o) - rr;
      if (jv) {
        const int i = k * n_obs + j;
        if (c < pmin) pmin = c;
        // (c == best_c == +inf is no tie: +inf never wins the strict `<`)
        if (c < best_c || (c == best_c && i < best_i && c < inf)) { best_c = c; best_i = i; }
        if (c < A.margin && k < viol) viol = k;
      }
    }
    if (A.per_obstacle) {
      for (int off = 32; off >= G; off >>= 1) {   // over the rows of the wave
        const double o = __shfl_xor(pmin, off);
        pmin = (o < pmin) ? o : pmin;
      }
      if (row == 0) s_po[wave][col] = pmin;
      __syncthreads();
      if (wave == 0 && row == 0 && jv) {
        double m = s_po[0][col];
#pragma unroll
        for (int w = 1; w < PMAF_AUDIT_WAVES; w++) { const double o = s_po[w][col]; m = (o < m) ? o : m; }
        A.per_obstacle[out * n_obs + j] = m;
      }
      __syncthreads();
    }
  }
  group_argmin<64>(best_c, best_i);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(viol, off);
    viol = (o < viol) ? o : viol;
  }
  if (lane == 0) { s_c[wave] = best_c; s_i[wave] = best_i; s_v[wave] = viol; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < PMAF_AUDIT_WAVES; w++) {
      const double oc = s_c[w];
      const int oi = s_i[w], ov = s_v[w];
      if (oc < best_c || (oc == best_c && oi < best_i)) { best_c = oc; best_i = oi; }
      viol = (ov < viol) ? ov : viol;
    }
    const bool found = best_i != 0x7fffffff;
    A.clearance[out] = best_c;
    if (A.step) A.step[out] = found ? best_i / n_obs : -1;
    if (A.obstacle) A.obstacle[out] = found ? best_i % n_obs : -1;
    if (A.first_violation) A.first_violation[out] = (viol == 0x7fffffff) ? n : viol;
  }
}

}  // namespace pmaf
