// pmaf_xaudit_kernels.hpp -- kernels of pmaf_cross_audit / pmaf_cross_audit_tracks / pmaf_select_pair (include/pmaf.h,
// "cross audit"): the predicted paths of one population held against a second path set -- another population of the
// handle (read where it lies, on the device) or tracks the caller uploaded -- step by step, and the cheapest pair of
// candidates that keeps its distance. SURVEY.md 8(e) names the other arm's "winning path, sampled at the same step"
// as the dual-arm coupling; the reference has nothing of the kind (its arms see one sphere at the other arm's
// set-point). Included by pmaf_k_misc.hip (no translation unit of its own).
//
// Semantics (the host-side contract is in include/pmaf.h): path i of set A has points x_0 .. x_{n-1}, path j of set B
// y_0 .. y_{m-1}, both on the handle's step grid; an ended path HOLDS its last point: xh_k = x_{min(k, n-1)},
// yh_k = y_{min(k, m-1)} for k < K = max(n, m).
//   d2(k)     = dot(xh_k - yh_k, xh_k - yh_k)      in the build's association, every operation rounded
//   step      = argmin_k d2(k) by strict `<` from +inf, k ascending (ties: the smallest k; a NaN never wins; -1: none)
//   clearance = sqrt(d2(step)) - separation        (+inf when nothing won or a path is empty; no floor, no cap)
//
// k_cross_audit   N_a * N_b * K independent point pairs of ~9 FP64 operations: unblocked that is six loads per
//                 pair-step, so it is blocked like a small GEMM over the tile of pmaf_cross_audit.hpp (ownership, LDS
//                 layout, staging and the hold rule are described there): both tiles' chunk is staged into LDS and a
//                 thread keeps one running (d2, k) for each of its 2 x 2 pairs -- 12 LDS reads for 4 pair-steps instead
//                 of 24 global ones. The loop is that header's xaudit_step_walk on the points as they lie (why a step
//                 past a pair's K never wins is said there).
//                  - 2 x 2 pairs x (d2, k) + 12 staged values: a small register block (resource report: no scratch),
//                    several waves per SIMD.
// k_pair_reduce   pmaf_select_pair: over the device-resident matrix and the two cost vectors, the minimum of
//                 S = cost_a[i] + cost_b[j] among the pairs with clearance >= margin and the maximum clearance of all
//                 pairs, each under the total order (value, i * N_b + j) -- what a row-major scan with a strict
//                 comparison finds. Two stages of the same block reduction (shuffles, then LDS across the waves):
//                 up to PMAF_XAUDIT_PARTIALS blocks write one partial each, one block folds them and writes the result.
#pragma once
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_cross_audit.hpp"

namespace pmaf {

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_cross_audit(CrossAuditArgs A) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  __shared__ double s_a[C * 3 * TP], s_b[C * 3 * TP];
  __shared__ int s_na[T], s_nb[T], s_k[1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  const int K = xaudit_tile_lengths(A, a0, b0, s_na, s_nb, s_k);
  const double inf = __builtin_huge_val();
  double best[2][2] = {{inf, inf}, {inf, inf}};
  int bk[2][2] = {{-1, -1}, {-1, -1}};
  xaudit_step_walk(A, a0, b0, K, s_a, s_b, s_na, s_nb, tx, ty, XAuditAsLies{}, XAuditAsLies{}, best, bk);
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int c = 0; c < 2; c++)
      xaudit_store_pair(A, a0, b0, ty + 16 * r, tx + 16 * c, s_na, s_nb, best[r][c], bk[r][c], -1, nullptr);
}

__device__ __forceinline__ void pair_fold(PairBest &b, double s, int si, double nc, int ci) {
  const bool ts = (s < b.s) || (s == b.s && si < b.si);
  b.s = ts ? s : b.s;
  b.si = ts ? si : b.si;
  const bool tc = (nc < b.nc) || (nc == b.nc && ci < b.ci);
  b.nc = tc ? nc : b.nc;
  b.ci = tc ? ci : b.ci;
}

// over the block's threads; the result is valid in thread 0
__device__ __forceinline__ void pair_block_reduce(PairBest &b) {
  __shared__ double s_s[PMAF_XAUDIT_THREADS / 64], s_c[PMAF_XAUDIT_THREADS / 64];
  __shared__ int s_si[PMAF_XAUDIT_THREADS / 64], s_ci[PMAF_XAUDIT_THREADS / 64];
  group_argmin<64>(b.s, b.si);
  group_argmin<64>(b.nc, b.ci);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_s[wave] = b.s; s_si[wave] = b.si; s_c[wave] = b.nc; s_ci[wave] = b.ci; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < PMAF_XAUDIT_THREADS / 64; w++) pair_fold(b, s_s[w], s_si[w], s_c[w], s_ci[w]);
}

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_pair_reduce(PairArgs A) {
  const double inf = __builtin_huge_val();
  PairBest b{inf, inf, 0x7fffffff, 0x7fffffff};
  const int total = A.n_a * A.n_b;
  // ascending indices per thread and a strict comparison: a thread keeps the smallest index of its best value
  for (int idx = blockIdx.x * PMAF_XAUDIT_THREADS + threadIdx.x; idx < total; idx += gridDim.x * PMAF_XAUDIT_THREADS) {
    const int i = idx / A.n_b, j = idx - i * A.n_b;
    const double c = A.clearance[idx];
    const double s = A.cost_a[i] + A.cost_b[j];
    if (c >= A.margin && s < b.s) { b.s = s; b.si = idx; }   // false for a NaN clearance, a NaN sum, a sum of +inf
    if (-c < b.nc) { b.nc = -c; b.ci = idx; }                // c > running maximum, from -inf; false for NaN
  }
  pair_block_reduce(b);
  if (threadIdx.x == 0) {
    PairBest *p = A.partial + blockIdx.x;
    *p = b;
  }
}

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_pair_final(PairArgs A, int n_partials) {
  const double inf = __builtin_huge_val();
  PairBest b{inf, inf, 0x7fffffff, 0x7fffffff};
  if ((int)threadIdx.x < n_partials) b = A.partial[threadIdx.x];
  pair_block_reduce(b);
  if (threadIdx.x == 0) {
    PairResult r;
    const double nan = __builtin_nan("");
    const int idx = b.si != 0x7fffffff ? b.si : b.ci;
    r.feasible = b.si != 0x7fffffff ? 1 : 0;
    if (idx != 0x7fffffff) {
      r.i = idx / A.n_b;
      r.j = idx - r.i * A.n_b;
      r.cost = A.cost_a[r.i] + A.cost_b[r.j];
      r.clearance = A.clearance[idx];
    } else {
      r.i = r.j = -1;
      r.cost = r.clearance = nan;
    }
    r.pad = 0;
    *A.result = r;
  }
}

}  // namespace pmaf
