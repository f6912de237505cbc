// pmaf_cross_audit.hpp -- kernels of pmaf_cross_audit / pmaf_cross_audit_tracks / pmaf_select_pair (include/pmaf.h,
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
//                 pair-step, so it is blocked like a small GEMM. A block of 256 threads owns a tile of T = 32 paths of A
//                 x T = 32 paths of B and walks the steps in chunks of C = 16: both tiles' chunk is staged into LDS,
//                 thread (ty, tx) = (tid / 16, tid % 16) keeps the 2 x 2 pairs (ty + 16 r, tx + 16 c) with one running
//                 (d2, k) each -- 12 LDS reads for 4 pair-steps instead of 24 global ones.
//                  - LDS layout: component-major rows s[k][xyz][T + 1] per tile (SoA; 2 x 16 x 3 x 33 doubles =
//                    24.8 KB per block, six blocks per CU). In the step loop the 16 lanes of a row read 16
//                    consecutive doubles of B (contiguous 128 B) and one double of A (broadcast): no bank conflicts in
//                    either half-wave.
//                  - staging: consecutive threads take consecutive doubles of a path's chunk (48 doubles = 384
//                    contiguous bytes of the 24-byte-stride AoS rows per path: coalesced) and store them T + 1 doubles
//                    apart -- the padding spreads those stores over the banks (stride 66 dwords = 2 mod 32), where a
//                    stride of T would put all of them on one.
//                  - the hold rule is an index clamp at staging time, min(k, n - 1), without a branch; steps past a
//                    pair's K (the block walks to the longest path of its tile) and past the ragged end of the last
//                    chunk repeat a held point, tie with an earlier step and so never win the strict `<`. Paths past
//                    the ragged edge of N_a / N_b are clamped to the last path (loaded, computed, not stored); an
//                    empty path stages its row 0 (inside the allocation, value irrelevant) and its pairs are
//                    overwritten with +inf / -1 at the end.
//                  - 2 x 2 pairs x (d2, k) + 12 staged values: a small register block (resource report: no scratch),
//                    several waves per SIMD. No reduction across threads at all -- a pair belongs to one thread -- so
//                    there are no atomics and the result does not depend on the tiling.
// k_pair_reduce   pmaf_select_pair: over the device-resident matrix and the two cost vectors, the minimum of
//                 S = cost_a[i] + cost_b[j] among the pairs with clearance >= margin and the maximum clearance of all
//                 pairs, each under the total order (value, i * N_b + j) -- what a row-major scan with a strict
//                 comparison finds. Two stages of the same block reduction (shuffles, then LDS across the waves):
//                 up to PMAF_XAUDIT_PARTIALS blocks write one partial each, one block folds them and writes the result.
#pragma once
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"

namespace pmaf {

#define PMAF_XAUDIT_TILE 32       // T: paths of A and of B per block (2 x 2 pairs per thread, 16 x 16 threads)
#define PMAF_XAUDIT_CHUNK 16      // C: steps staged per pass
#define PMAF_XAUDIT_THREADS 256

// one tile's chunk of steps [k0, k0 + C) into s[(k * 3 + c) * (T + 1) + path]
__device__ __forceinline__ void xaudit_stage(double *s, const double *paths, const int *s_n, int first, int count,
                                             int cap, int k0) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  for (int e = threadIdx.x; e < T * C * 3; e += PMAF_XAUDIT_THREADS) {
    const int t = e / (C * 3), r = e - t * (C * 3);
    const int k = r / 3, c = r - k * 3;
    int p = first + t;
    p = p < count ? p : count - 1;            // ragged edge of the set: the last path again (never stored)
    int kk = k0 + k;
    const int last = s_n[t] - 1;
    kk = kk < last ? kk : last;               // hold: an ended path stays at its last point
    kk = kk > 0 ? kk : 0;                     // (an empty path: row 0, overwritten at the end)
    PMAF_BOUND(p >= 0 && kk < cap);
    s[r * TP + t] = paths[((size_t)p * cap + kk) * 3 + c];
  }
}

#ifndef PMAF_XAUDIT_NO_KERNELS   // pmaf_k_slack.hip shares the tile constants and xaudit_stage, not the kernels
__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_cross_audit(CrossAuditArgs A) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  __shared__ double s_a[C * 3 * TP], s_b[C * 3 * TP];
  __shared__ int s_na[T], s_nb[T], s_k[1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  if (tid < 2 * T) {   // wave 0: the tile's path lengths and the longest of them
    const int t = tid & (T - 1);
    const bool is_b = tid >= T;
    int p = (is_b ? b0 : a0) + t;
    const int count = is_b ? A.n_b : A.n_a;
    p = p < count ? p : count - 1;
    int n = (is_b ? A.len_b : A.len_a)[p];
    PMAF_BOUND(n >= 0 && n <= A.cap);
    n = n < A.cap ? n : A.cap;
    n = n > 0 ? n : 0;
    (is_b ? s_nb : s_na)[t] = n;
    int m = n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(m, off);
      m = o > m ? o : m;
    }
    if (tid == 0) s_k[0] = m;
  }
  __syncthreads();
  const int K = s_k[0];
  const double inf = __builtin_huge_val();
  double best[2][2] = {{inf, inf}, {inf, inf}};
  int bk[2][2] = {{-1, -1}, {-1, -1}};
  for (int k0 = 0; k0 < K; k0 += C) {   // block-uniform trip count
    xaudit_stage(s_a, A.paths_a, s_na, a0, A.n_a, A.cap, k0);
    xaudit_stage(s_b, A.paths_b, s_nb, b0, A.n_b, A.cap, k0);
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < C; k++) {
      const double *ra = s_a + k * 3 * TP + ty, *rb = s_b + k * 3 * TP + tx;
      V3 x[2], y[2];
#pragma unroll
      for (int r = 0; r < 2; r++) {
        x[r] = mk(ra[16 * r], ra[TP + 16 * r], ra[2 * TP + 16 * r]);
        y[r] = mk(rb[16 * r], rb[TP + 16 * r], rb[2 * TP + 16 * r]);
      }
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
          const V3 d = x[r] - y[c];
          const double d2 = dot(d, d);
          const bool take = d2 < best[r][c];   // strict, k ascending: ties keep the smallest k, a NaN never wins
          best[r][c] = take ? d2 : best[r][c];
          bk[r][c] = take ? k0 + k : bk[r][c];
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int ti = ty + 16 * r, tj = tx + 16 * c;
      const int i = a0 + ti, j = b0 + tj;
      if (i < A.n_a && j < A.n_b) {
        const bool won = bk[r][c] >= 0 && s_na[ti] > 0 && s_nb[tj] > 0;
        const size_t o = (size_t)i * A.n_b + j;
        A.clearance[o] = won ? __builtin_sqrt(best[r][c]) - A.separation : inf;
        if (A.step) A.step[o] = won ? bk[r][c] : -1;
      }
    }
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
#endif  // PMAF_XAUDIT_NO_KERNELS

}  // namespace pmaf
