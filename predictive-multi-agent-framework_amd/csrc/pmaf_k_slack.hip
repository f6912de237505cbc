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
//                 every pair's K x K table. Ownership, LDS layout and staging are the tile's, the loop is xaudit_band_walk
//                 on the points as they lie (pmaf_cross_audit.hpp: the chunk pairs, the edge diagonals, the tie rule
//                 and why a step past a pair's K cannot win are said there, once for both banded kernels); a thread
//                 keeps one running (d2, k, l) for each of its 2 x 2 pairs.
//                  - resources (build's report): 86 VGPRs, no scratch, 25 608 B LDS, 5 waves per SIMD.
//                  - empty paths and the ragged edge of N_a / N_b: the tile's rule (xaudit_store_pair: +inf / -1 / -1).
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_cross_audit.hpp"

using namespace pmaf;

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_cross_audit_slack(CrossAuditSlackArgs S) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  __shared__ double s_a[C * 3 * TP], s_b[C * 3 * TP];
  __shared__ int s_na[T], s_nb[T], s_k[1];
  const CrossAuditArgs &A = S.X;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  const int late_a = S.late_a, late_b = S.late_b;
  const int K = xaudit_tile_lengths(A, a0, b0, s_na, s_nb, s_k);
  const double inf = __builtin_huge_val();
  double best[2][2] = {{inf, inf}, {inf, inf}};
  int bk[2][2] = {{-1, -1}, {-1, -1}}, bl[2][2] = {{-1, -1}, {-1, -1}};
  xaudit_band_walk(A, a0, b0, K, late_a, late_b, s_a, s_b, s_na, s_nb, tx, ty, XAuditAsLies{}, XAuditAsLies{}, best, bk, bl);
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int c = 0; c < 2; c++)
      xaudit_store_pair(A, a0, b0, ty + 16 * r, tx + 16 * c, s_na, s_nb, best[r][c], bk[r][c], bl[r][c], S.step_b);
}

void pmaf_k_launch_cross_audit_slack(const CrossAuditSlackArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_cross_audit_slack, xaudit_grid(A.X), dim3(PMAF_XAUDIT_THREADS), 0, s, A);
}
