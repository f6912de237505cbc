// pmaf_cross_audit.hpp -- the cross audit's tile, what its four kernels share: k_cross_audit (pmaf_xaudit_kernels.hpp,
// compiled in pmaf_k_misc.hip), k_cross_audit_slack (pmaf_k_slack.hip), k_cross_audit_attached (pmaf_k_xattach.hip) and
// k_xaudit_attached_slack (pmaf_k_xattach_slack.hip). All own the same tile and differ only in the steps of B a step
// of A is held against and in what is staged of a point (the attached audits: the sphere that rides on it); this header has the tile's shape (the constants the GPU tests read their
// shapes from), its staging into LDS, its prologue and the store of one finished pair. No kernel is defined here.
//
// Tile          a block of 256 threads owns T = 32 paths of A x T = 32 paths of B and walks the steps in chunks of
//               C = 16; thread (ty, tx) = (tid / 16, tid % 16) keeps the 2 x 2 pairs (ty + 16 r, tx + 16 c). A pair
//               belongs to one thread: no reduction across threads, no atomics, a result that does not depend on the
//               tiling.
//  - LDS layout: component-major rows s[k][xyz][T + 1] per tile (SoA; 2 x 16 x 3 x 33 doubles = 24.8 KB per block, six
//    blocks per CU). In the step loop the 16 lanes of a row read 16 consecutive doubles of B (contiguous 128 B) and one
//    double of A (broadcast): no bank conflicts in either half-wave.
//  - staging (xaudit_stage): consecutive threads take consecutive doubles of a path's chunk (48 doubles = 384
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
// component c of a point (k_cross_audit_attached, pmaf_k_xattach.hip: the sphere that rides on the point)
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

// ... the points as they lie
__device__ __forceinline__ void xaudit_stage(double *s, const double *paths, const int *s_n, int first, int count,
                                             int cap, int k0) {
  xaudit_stage_with(s, paths, s_n, first, count, cap, k0, [](double v, int) { return v; });
}

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

}  // namespace pmaf
