// pmaf_k_slack.hip -- k_cross_audit_slack, the kernel of pmaf_cross_audit_slack / pmaf_cross_audit_tracks_slack /
// pmaf_select_pair_slack (include/pmaf.h, "cross audit with timing slack"), and its launcher. A translation unit of its
// own: the code objects of the other units -- the rollout kernels, k_manager and k_cross_audit in pmaf_k_misc.hip --
// stay byte for byte what they were (NOTES.md 1: code placement alone moves the rollout loop).
//
// Semantics (the host-side contract is in include/pmaf.h): the cross audit's two path sets, hold rule and d2, but the
// two arms need not be at the same step: A may run up to late_a steps behind B's clock, B up to late_b behind A's.
//   admitted (k, l), 0 <= k, l < K = max(n, m):  -late_b <= l - k <= late_a
//   d2(k, l)          = dot(xh_k - yh_l, xh_k - yh_l)   in the build's association, every operation rounded
//   (step_a, step_b)  = the admitted pair that is least under the total order (d2, k, l): what a scan with k ascending,
//                       then l ascending, and a strict `<` from +inf finds (a NaN never wins; (-1, -1): none won)
//   clearance         = sqrt(d2(step_a, step_b)) - separation   (+inf when nothing won or a path is empty)
//
// k_cross_audit_slack   N_a * N_b * K * (late_a + late_b + 1) independent pair-steps, a band around the diagonal of
//                 every pair's K x K table. Ownership, LDS layout and staging are the tile's (pmaf_cross_audit.hpp, shared
//                 with k_cross_audit); a thread keeps one running (d2, k, l) for each of its 2 x 2 pairs.
//                  - LDS does not depend on the slack: one chunk of C = 16 steps of A and one of B in the tile's layout
//                    (24.8 KB per block, as in k_cross_audit). For every chunk [k0, k0 + C) of A the
//                    block walks the chunks of B, on the same grid of multiples of C, that meet the band
//                    [k0 - late_b, k0 + C - 1 + late_a] clipped to [0, K): A's chunk is staged once, B's once per
//                    chunk pair (6 global loads per thread against up to 4 C^2 = 1024 pair-steps).
//                  - a chunk pair does up to C x C pair-steps per pair: row k's two points of A in registers, the l
//                    loop reads the two points of B (6 LDS reads for 4 pair-steps; B: 16 consecutive doubles per
//                    half-wave row, A: a broadcast -- no bank conflicts). A chunk pair that lies wholly inside the band
//                    runs the full C x C loop. At the two edge diagonals the band is no per-lane mask either: k, l0
//                    and the slacks are block-uniform, so it is the l loop's BOUNDS, max(l0, k - late_b) ..
//                    min(l0 + C - 1, k + late_a), and no lane computes a pair-step that is not admitted by the band.
//                  - tie rule. The traversal (chunk of A, chunk of B, k, l) is not the order (k, l). For two visited
//                    steps e (earlier) and c (later), (k_c, l_c) < (k_e, l_e) lexicographically iff k_c < k_e: with
//                    k_c == k_e both lie in one chunk of A, and c then comes from a later chunk of B or from the same
//                    chunk pair further along l, so l_c > l_e. Hence
//                        take = (d2 < best) | ((d2 == best) & (k < best_k))
//                    keeps exactly the least visited step under (d2, k, l): one integer compare on top of the strict
//                    `<`, false for a NaN on either side, false against the initial (+inf, -1, -1). Held path ends make
//                    exact ties the normal case, so the condition is evaluated without a branch.
//                  - resources (build's report): 86 VGPRs, no scratch, 25 608 B LDS, 5 waves per SIMD. The l loop is
//                    unrolled by 2: by 4 the max-ilp schedule takes 136 VGPRs (3 waves per SIMD).
//                  - the hold rule is xaudit_stage's index clamp. Steps past a pair's own K = max(n, m) are visited
//                    where a longer neighbour of the tile (or the ragged last chunk) makes the block walk further.
//                    Such a step (k, l), max(k, l) >= K, cannot win: let k' = min(k, K - 1), l' = min(l, K - 1). Both
//                    paths have ended by K - 1, so xh_k' = xh_k and yh_l' = yh_l: d2(k', l') has the same bits.
//                    (k', l') is admitted: both clipped gives (K - 1, K - 1); only k clipped gives l - k' <= 0 <=
//                    late_a and l - k' > l - k >= -late_b; only l clipped the mirror image. And (k', l') < (k, l). So
//                    every such step ties with (or, NaN, loses like) an ADMITTED step of a smaller (k, l) that the
//                    block also visits, and the order above never prefers it.
//                  - empty paths and the ragged edge of N_a / N_b: the tile's rule (xaudit_store_pair: +inf / -1 / -1).
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_cross_audit.hpp"

using namespace pmaf;

// the two points of B at staged row l against the two of A in registers: 4 pair-steps
__device__ __forceinline__ void xslack_row(const V3 (&x)[2], const double *rb, int kk, int ll, double (&best)[2][2],
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
      // least under (d2, k, l): a later step of the traversal has a smaller (k, l) iff its k is smaller (see above)
      // (bitwise, not short-circuit: three compares and two mask operations, no branch on the lanes that tie)
      const bool take = (d2 < best[r][c]) | ((d2 == best[r][c]) & (kk < bk[r][c]));
      best[r][c] = take ? d2 : best[r][c];
      bk[r][c] = take ? kk : bk[r][c];
      bl[r][c] = take ? ll : bl[r][c];
    }
}

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_cross_audit_slack(CrossAuditSlackArgs S) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  __shared__ double s_a[C * 3 * TP], s_b[C * 3 * TP];
  __shared__ int s_na[T], s_nb[T], s_k[1];
  const CrossAuditArgs &A = S.X;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  const int late_a = S.late_a, late_b = S.late_b;
  const int K = xaudit_tile_lengths(A, a0, b0, s_na, s_nb, s_k);
  PMAF_BOUND(late_a >= 0 && late_a <= A.cap && late_b >= 0 && late_b <= A.cap);
  const double inf = __builtin_huge_val();
  double best[2][2] = {{inf, inf}, {inf, inf}};
  int bk[2][2] = {{-1, -1}, {-1, -1}}, bl[2][2] = {{-1, -1}, {-1, -1}};
  for (int k0 = 0; k0 < K; k0 += C) {   // every trip count below is block-uniform
    xaudit_stage(s_a, A.paths_a, s_na, a0, A.n_a, A.cap, k0);
    // the steps of B this chunk of A can meet, and the chunks (multiples of C) that hold them
    int lo = k0 - late_b;
    lo = lo > 0 ? lo : 0;
    int hi = k0 + C - 1 + late_a;
    hi = hi < K - 1 ? hi : K - 1;
    for (int l0 = lo - lo % C; l0 <= hi; l0 += C) {
      xaudit_stage(s_b, A.paths_b, s_nb, b0, A.n_b, A.cap, l0);
      __syncthreads();
      // the extreme differences l - k of the chunk pair
      const bool inside = l0 + C - 1 - k0 <= late_a && l0 - (k0 + C - 1) >= -late_b;
      if (inside) {
        for (int k = 0; k < C; k++) {
          const double *ra = s_a + k * 3 * TP + ty;
          const V3 x[2] = {mk(ra[0], ra[TP], ra[2 * TP]), mk(ra[16], ra[TP + 16], ra[2 * TP + 16])};
#pragma unroll 2
          for (int l = 0; l < C; l++) xslack_row(x, s_b + l * 3 * TP + tx, k0 + k, l0 + l, best, bk, bl);
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
          for (int ll = l_lo; ll <= l_hi; ll++) xslack_row(x, s_b + (ll - l0) * 3 * TP + tx, kk, ll, best, bk, bl);
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int c = 0; c < 2; c++)
      xaudit_store_pair(A, a0, b0, ty + 16 * r, tx + 16 * c, s_na, s_nb, best[r][c], bk[r][c], bl[r][c], S.step_b);
}

void pmaf_k_launch_cross_audit_slack(const CrossAuditSlackArgs &A, hipStream_t s) {
  const dim3 grid((unsigned)((A.X.n_b + PMAF_XAUDIT_TILE - 1) / PMAF_XAUDIT_TILE),
                  (unsigned)((A.X.n_a + PMAF_XAUDIT_TILE - 1) / PMAF_XAUDIT_TILE));
  hipLaunchKernelGGL(k_cross_audit_slack, grid, dim3(PMAF_XAUDIT_THREADS), 0, s, A);
}
