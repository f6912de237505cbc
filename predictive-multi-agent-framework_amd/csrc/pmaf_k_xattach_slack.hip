// pmaf_k_xattach_slack.hip -- k_xaudit_attached_slack, the kernel of pmaf_cross_audit_attached_slack and of the pair
// side of pmaf_select_pair_clear_tracked_slack (include/pmaf.h, "joint selection on coupled handles with timing slack"),
// and its launcher. A translation unit of its own, object xattach_slack.o: the code objects of the other units -- the
// rollout kernels, k_cross_audit in pmaf_k_misc.hip, k_cross_audit_slack, k_cross_audit_attached -- stay byte for byte
// what they were (NOTES.md 1: code placement alone moves the rollout loop). The kernel's name carries neither
// "k_cross_audit_attached" nor "k_cross_audit_slack": the resource-record tests of those two kernels
// (tests/test_attached_audit.py, tests/test_slack_audit.py) find theirs by these substrings of the mangled names.
//
// Semantics (the host-side contract is in include/pmaf.h): the product of the attached audit's TERMS and the slacked
// audit's BAND. k is always A's step and l always B's; M = n_obs - 1; src / scale / anchor = the handle's current
// coupling, r = the staged list's radii.
//   admitted (k, l), 0 <= k, l < K = max(n, m):  -late_b <= l - k <= late_a
//   term 0          u = xh_k, z = yh_l,                                              R = separation
//   term 1 + s      src[a][s] == b:  u = xh_k, z = RN(anchor[a][s] + RN(scale[a][s] * yh_l)),  R = RN(radius + r[a][s])
//                   (the sphere is a part of arm B: it is on B's clock)
//   term 1 + M + s  src[b][s] == a:  u = yh_l, z = RN(anchor[b][s] + RN(scale[b][s] * xh_k)),  R = RN(radius + r[b][s])
//   d2_t   = the least dot(u - z, u - z) over the admitted pairs under the total order (d2, k, l): a scan with k, then l
//            ascending and a strict `<` from +inf (a NaN never wins)
//   gap_t  = sqrt(d2_t) - R_t
//   clearance = min over t of gap_t, strict `<` in term order: ties go to the smallest term, then to that term's least
//   (k, l); (step_a, step_b) and sphere are the winning term's; +inf / -1 / -1 / -1 when nothing won or a path is empty.
//
// k_xaudit_attached_slack   the product of two shared pieces on the tile of pmaf_cross_audit.hpp: terms outermost
//                 (pmaf_xattach_terms.hpp: the loop over the terms, the ride, the fold and the store, shared with
//                 k_cross_audit_attached), xaudit_band_walk inside a term (pmaf_cross_audit.hpp, shared with
//                 k_cross_audit_slack: the chunk pairs, the edge diagonals, the tie rule inside a term and why a step
//                 past a pair's K cannot win a term are said there).
//                  - the ride is applied AT STAGING (XAttachRide through xaudit_stage_with): to A's chunk for a term
//                    1 + M + s, to every chunk of B for a term 1 + s. A's chunk is therefore transformed once per term
//                    and k0, B's once per chunk PAIR (a chunk of B is restaged for every chunk of A that meets it: 6
//                    flops per staged double against up to 4 C^2 pair-steps per thread). The step loop is d = a - b on
//                    the two staged tiles. For the terms 1 + M + s that is z - yh_l, the negation of the contract's d:
//                    every component's square, and so dot(d, d) in either association, has the same bits.
//                  - at the end of a term the thread folds (d2, k, l) of each of its 2 x 2 pairs into the pair's running
//                    (gap, k, l, t): one sqrt per pair and term; the strict `<` in term order is the tie rule across
//                    terms.
//                  - LDS: two tiles of one chunk plus the lengths, 25 608 B per block, independent of the slack and of
//                    the number of terms; no atomics, a pair belongs to one thread, the result does not depend on the
//                    grid.
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_cross_audit.hpp"
#include "pmaf_xattach.hpp"
#include "pmaf_xattach_terms.hpp"

using namespace pmaf;

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_xaudit_attached_slack(CrossAuditAttachedSlackArgs S) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  __shared__ double s_a[C * 3 * TP], s_b[C * 3 * TP];
  __shared__ int s_na[T], s_nb[T], s_k[1];
  const CrossAuditArgs &A = S.T.X;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  const int late_a = S.late_a, late_b = S.late_b;
  const int K = xaudit_tile_lengths(A, a0, b0, s_na, s_nb, s_k);
  const double inf = __builtin_huge_val();
  XAttachBest p00, p01, p10, p11;   // the four pairs' running (gap, k, l, t): named, an array changed the kernel's code
  xattach_for_each_term(S.T, [&](int t, const XAttachRide fa, const XAttachRide fb, double R) {
    double best[2][2] = {{inf, inf}, {inf, inf}};
    int bk[2][2] = {{-1, -1}, {-1, -1}}, bl[2][2] = {{-1, -1}, {-1, -1}};
    xaudit_band_walk(A, a0, b0, K, late_a, late_b, s_a, s_b, s_na, s_nb, tx, ty, fa, fb, best, bk, bl);
    p00.fold(best[0][0], bk[0][0], bl[0][0], R, t);
    p01.fold(best[0][1], bk[0][1], bl[0][1], R, t);
    p10.fold(best[1][0], bk[1][0], bl[1][0], R, t);
    p11.fold(best[1][1], bk[1][1], bl[1][1], R, t);
  });
  xattach_store_pair(S.T, a0, b0, ty, tx, s_na, s_nb, p00, S.step_b);
  xattach_store_pair(S.T, a0, b0, ty, tx + 16, s_na, s_nb, p01, S.step_b);
  xattach_store_pair(S.T, a0, b0, ty + 16, tx, s_na, s_nb, p10, S.step_b);
  xattach_store_pair(S.T, a0, b0, ty + 16, tx + 16, s_na, s_nb, p11, S.step_b);
}

void pmaf_k_launch_cross_audit_attached_slack(const CrossAuditAttachedSlackArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_xaudit_attached_slack, xaudit_grid(A.T.X), dim3(PMAF_XAUDIT_THREADS), 0, s, A);
}
