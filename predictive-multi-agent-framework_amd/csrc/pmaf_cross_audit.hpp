// pmaf_cross_audit.hpp -- the cross audit's tile and the two walks over it: what the audit's four kernels are made of.
//                  | one term (end effectors)                       | the attached terms (pmaf_xattach_terms.hpp)
//   step with step | k_cross_audit (pmaf_xaudit_kernels.hpp,        | k_cross_audit_attached (pmaf_k_xattach.hip)
//                  |   compiled in pmaf_k_misc.hip)                 |
//   band of steps  | k_cross_audit_slack (pmaf_k_slack.hip)         | k_xaudit_attached_slack (pmaf_k_xattach_slack.hip)
// All own the same tile. A row of the table is one walk (xaudit_step_walk, xaudit_band_walk: the steps of B a step of A
// is held against); a column is what is staged of a point (as it lies, or the sphere that rides on it). Included by
// pmaf_xaudit_kernels.hpp and by the three .hip units above. This header has the tile's shape (the constants the GPU
// tests read their shapes from), its staging into LDS, its prologue, the walks, the store of one finished pair and the
// launch grid. No kernel is defined here.
//
// Tile          a block of 256 threads owns T = 32 paths of A x T = 32 paths of B and walks the steps in chunks of
//               C = 16; thread (ty, tx) = (tid / 16, tid % 16) keeps the 2 x 2 pairs (ty + 16 r, tx + 16 c). A pair
//               belongs to one thread: no reduction across threads, no atomics, a result that does not depend on the
//               tiling.
//  - LDS layout: component-major rows s[k][xyz][T + 1] per tile (SoA; 2 x 16 x 3 x 33 doubles = 24.8 KB per block, six
//    blocks per CU). In the step loop the 16 lanes of a row read 16 consecutive doubles of B (contiguous 128 B) and one
//    double of A (broadcast): no bank conflicts in either half-wave.
//  - staging (xaudit_stage_with): consecutive threads take consecutive doubles of a path's chunk (48 doubles = 384
//    contiguous bytes of the 24-byte-stride AoS rows per path: coalesced) and store them T + 1 doubles apart -- the
//    padding spreads those stores over the banks (stride 66 dwords = 2 mod 32), where a stride of T would put all of
//    them on one.
//  - the hold rule is an index clamp at staging time, min(k, n - 1), without a branch. Paths past the ragged edge of
//    N_a / N_b are clamped to the last path (loaded, computed, not stored); an empty path stages its row 0 (inside the
//    allocation, value irrelevant) and its pairs are overwritten with +inf / -1 at the end (xaudit_store_pair).
#pragma once
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"

namespace pmaf {

#define PMAF_XAUDIT_TILE 32       // T: paths of A and of B per block (2 x 2 pairs per thread, 16 x 16 threads)
#define PMAF_XAUDIT_CHUNK 16      // C: steps staged per pass
#define PMAF_XAUDIT_THREADS 256

// one tile's chunk of steps [k0, k0 + C) into s[(k * 3 + c) * (T + 1) + path]; f(value, c) is what is stored of
// component c of a point (XAuditAsLies below; the attached audits: the sphere that rides on the point, XAttachRide)
template <typename F>
__device__ __forceinline__ void xaudit_stage_with(double *s, const double *paths, const int *s_n, int first, int count,
                                                  int cap, int k0, F f) {
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
    s[r * TP + t] = f(paths[((size_t)p * cap + kk) * 3 + c], c);
  }
}

// ... the points as they lie: the staging functor of the two kernels without attached terms
struct XAuditAsLies {
  __device__ __forceinline__ double operator()(double v, int) const { return v; }
};

// the prologue: the clamped path lengths of the tile at (a0, b0) into s_na / s_nb [T], the longest of them -- the
// number of steps the block walks -- into s_k[0] and, behind a barrier, back to every thread
__device__ __forceinline__ int xaudit_tile_lengths(const CrossAuditArgs &A, int a0, int b0, int *s_na, int *s_nb, int *s_k) {
  constexpr int T = PMAF_XAUDIT_TILE;
  const int tid = threadIdx.x;
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
  return s_k[0];
}

// The step walk: step k of A against step k of B, k < K in chunks of C; lowers best / bk to each of the thread's 2 x 2
// pairs' least d2 and its step. The CALLER hands them in as +inf / -1 (nothing won yet; why: beside the band walk).
// fa / fb: what is staged of a point of A / of B. Steps past a pair's own K (the block walks to the longest path of its
// tile) and past the ragged end of the last chunk repeat a held point in both tiles, tie with an earlier step and so
// never win the strict `<` (the band walk's argument, one diagonal).
template <typename FA, typename FB>
__device__ __forceinline__ void xaudit_step_walk(const CrossAuditArgs &A, int a0, int b0, int K, double *s_a, double *s_b,
                                                 const int *s_na, const int *s_nb, int tx, int ty, FA fa, FB fb,
                                                 double (&best)[2][2], int (&bk)[2][2]) {
  constexpr int C = PMAF_XAUDIT_CHUNK, TP = PMAF_XAUDIT_TILE + 1;
  for (int k0 = 0; k0 < K; k0 += C) {   // block-uniform trip count
    xaudit_stage_with(s_a, A.paths_a, s_na, a0, A.n_a, A.cap, k0, fa);
    xaudit_stage_with(s_b, A.paths_b, s_nb, b0, A.n_b, A.cap, k0, fb);
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
}

// the band walk's row: the two points of B at staged row l against the two of A in registers, 4 pair-steps
__device__ __forceinline__ void xaudit_band_row(const V3 (&x)[2], const double *rb, int kk, int ll, double (&best)[2][2],
                                                int (&bk)[2][2], int (&bl)[2][2]) {
  constexpr int TP = PMAF_XAUDIT_TILE + 1;
  V3 y[2];
#pragma unroll
  for (int c = 0; c < 2; c++) y[c] = mk(rb[16 * c], rb[TP + 16 * c], rb[2 * TP + 16 * c]);
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const V3 d = x[r] - y[c];
      const double d2 = dot(d, d);
      // least under (d2, k, l): a later step of the traversal has a smaller (k, l) iff its k is smaller (tie rule below)
      // (bitwise, not short-circuit: three compares and two mask operations, no branch on the lanes that tie)
      const bool take = (d2 < best[r][c]) | ((d2 == best[r][c]) & (kk < bk[r][c]));
      best[r][c] = take ? d2 : best[r][c];
      bk[r][c] = take ? kk : bk[r][c];
      bl[r][c] = take ? ll : bl[r][c];
    }
}

// The band walk: step k of A against the steps l of B with -late_b <= l - k <= late_a, 0 <= k, l < K; lowers best / bk /
// bl to each of the thread's 2 x 2 pairs' least step under the total order (d2, k, l). The CALLER hands them in as
// +inf / -1 / -1 (nothing won yet): set inside this walk, the same values gave k_cross_audit_slack another register
// allocation (90 VGPRs for 86, 49 disassembly lines more; profiles/xaudit_shared_walks.md), and the step walk follows
// suit. fa / fb: what is staged of a point of A / of B.
//  - for every chunk [k0, k0 + C) of A the block walks the chunks of B, on the same grid of multiples of C, that meet the
//    band [k0 - late_b, k0 + C - 1 + late_a] clipped to [0, K): A's chunk is staged once, B's once per chunk pair (6
//    global loads per thread against up to 4 C^2 = 1024 pair-steps). LDS does not depend on the slack.
//  - a chunk pair does up to C x C pair-steps per pair: row k's two points of A in registers, the l loop reads the two
//    points of B (6 LDS reads for 4 pair-steps; B: 16 consecutive doubles per half-wave row, A: a broadcast -- no bank
//    conflicts). A chunk pair that lies wholly inside the band runs the full C x C loop. At the two edge diagonals the
//    band is no per-lane mask either: k, l0 and the slacks are block-uniform, so it is the l loop's BOUNDS, max(l0, k -
//    late_b) .. min(l0 + C - 1, k + late_a), and no lane computes a pair-step that is not admitted by the band.
//  - the l loop is unrolled by 2: by 4 the max-ilp schedule of k_cross_audit_slack takes 136 VGPRs (3 waves per SIMD).
//  - tie rule. The traversal (chunk of A, chunk of B, k, l) is not the order (k, l). For two visited steps e (earlier)
//    and c (later), (k_c, l_c) < (k_e, l_e) lexicographically iff k_c < k_e: with k_c == k_e both lie in one chunk of A,
//    and c then comes from a later chunk of B or from the same chunk pair further along l, so l_c > l_e. Hence
//        take = (d2 < best) | ((d2 == best) & (k < best_k))
//    keeps exactly the least visited step under (d2, k, l): one integer compare on top of the strict `<`, false for a
//    NaN on either side, false against the initial (+inf, -1, -1). Held path ends make exact ties the normal case, so
//    the condition is evaluated without a branch.
//  - the hold rule is xaudit_stage_with's index clamp. Steps past a pair's own K = max(n, m) are visited where a longer
//    neighbour of the tile (or the ragged last chunk) makes the block walk further. Such a step (k, l), max(k, l) >= K,
//    cannot win: let k' = min(k, K - 1), l' = min(l, K - 1). Both paths have ended by K - 1, so xh_k' = xh_k and
//    yh_l' = yh_l, and what a functor stages of a held point is what it staged of the point (the same operations on the
//    same bits): d2(k', l') has the same bits. (k', l') is admitted: both clipped gives (K - 1, K - 1); only k clipped
//    gives l - k' <= 0 <= late_a and l - k' > l - k >= -late_b; only l clipped the mirror image. And (k', l') < (k, l).
//    So every such step ties with (or, NaN, loses like) an ADMITTED step of a smaller (k, l) that the block also visits
//    in the same walk, and the order above never prefers it.
template <typename FA, typename FB>
__device__ __forceinline__ void xaudit_band_walk(const CrossAuditArgs &A, int a0, int b0, int K, int late_a, int late_b,
                                                 double *s_a, double *s_b, const int *s_na, const int *s_nb, int tx, int ty,
                                                 FA fa, FB fb, double (&best)[2][2], int (&bk)[2][2], int (&bl)[2][2]) {
  constexpr int C = PMAF_XAUDIT_CHUNK, TP = PMAF_XAUDIT_TILE + 1;
  PMAF_BOUND(late_a >= 0 && late_a <= A.cap && late_b >= 0 && late_b <= A.cap);
  for (int k0 = 0; k0 < K; k0 += C) {   // every trip count below is block-uniform
    xaudit_stage_with(s_a, A.paths_a, s_na, a0, A.n_a, A.cap, k0, fa);
    // the steps of B this chunk of A can meet, and the chunks (multiples of C) that hold them: lo <= k0 <= hi, so the
    // loop below runs at least once and its barriers order this chunk of A too
    int lo = k0 - late_b;
    lo = lo > 0 ? lo : 0;
    int hi = k0 + C - 1 + late_a;
    hi = hi < K - 1 ? hi : K - 1;
    for (int l0 = lo - lo % C; l0 <= hi; l0 += C) {
      xaudit_stage_with(s_b, A.paths_b, s_nb, b0, A.n_b, A.cap, l0, fb);
      __syncthreads();
      // the extreme differences l - k of the chunk pair
      const bool inside = l0 + C - 1 - k0 <= late_a && l0 - (k0 + C - 1) >= -late_b;
      if (inside) {
        for (int k = 0; k < C; k++) {
          const double *ra = s_a + k * 3 * TP + ty;
          const V3 x[2] = {mk(ra[0], ra[TP], ra[2 * TP]), mk(ra[16], ra[TP + 16], ra[2 * TP + 16])};
#pragma unroll 2
          for (int l = 0; l < C; l++) xaudit_band_row(x, s_b + l * 3 * TP + tx, k0 + k, l0 + l, best, bk, bl);
        }
      } else {
        for (int k = 0; k < C; k++) {
          const int kk = k0 + k;
          int l_lo = kk - late_b, l_hi = kk + late_a;
          l_lo = l_lo > l0 ? l_lo : l0;
          l_hi = l_hi < l0 + C - 1 ? l_hi : l0 + C - 1;
          if (l_lo > l_hi) continue;
          const double *ra = s_a + k * 3 * TP + ty;
          const V3 x[2] = {mk(ra[0], ra[TP], ra[2 * TP]), mk(ra[16], ra[TP + 16], ra[2 * TP + 16])};
          for (int ll = l_lo; ll <= l_hi; ll++) xaudit_band_row(x, s_b + (ll - l0) * 3 * TP + tx, kk, ll, best, bk, bl);
        }
      }
      __syncthreads();
    }
  }
}

// the epilogue of ONE pair (ti, tj) of the tile: its running minimum d2 at step k of A (and, slacked, step l of B;
// k < 0: nothing won) becomes clearance and step(s); an empty path on either side gives +inf / -1. step_b: the slacked
// audit's second step matrix, or nullptr.
__device__ __forceinline__ void xaudit_store_pair(const CrossAuditArgs &A, int a0, int b0, int ti, int tj, const int *s_na,
                                                  const int *s_nb, double d2, int k, int l, int32_t *step_b) {
  const int i = a0 + ti, j = b0 + tj;
  if (i < A.n_a && j < A.n_b) {
    const bool won = k >= 0 && s_na[ti] > 0 && s_nb[tj] > 0;
    const size_t o = (size_t)i * A.n_b + j;
    A.clearance[o] = won ? __builtin_sqrt(d2) - A.separation : __builtin_huge_val();
    if (A.step) A.step[o] = won ? k : -1;
    if (step_b) step_b[o] = won ? l : -1;
  }
}

// the four kernels' launch grid: one block per tile, B's tiles along x
static inline dim3 xaudit_grid(const CrossAuditArgs &A) {
  return dim3((unsigned)((A.n_b + PMAF_XAUDIT_TILE - 1) / PMAF_XAUDIT_TILE),
              (unsigned)((A.n_a + PMAF_XAUDIT_TILE - 1) / PMAF_XAUDIT_TILE));
}

}  // namespace pmaf
