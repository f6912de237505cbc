// pmaf_k_xattach.hip -- k_cross_audit_attached, the kernel of pmaf_cross_audit_attached and of the pair side of
// pmaf_select_pair_clear_tracked (include/pmaf.h, "joint selection on coupled handles"), and its launcher. A translation
// unit of its own, object xattach.o: the code objects of the other units -- the rollout kernels, k_cross_audit in
// pmaf_k_misc.hip, k_cross_audit_slack -- stay byte for byte what they were (NOTES.md 1: code placement alone moves the
// rollout loop).
//
// Semantics (the host-side contract is in include/pmaf.h): the cross audit's two path sets, hold rule and d2, but a pair
// (i, j) is held to several spheres, its TERMS, in this order (M = n_obs - 1; src / scale / anchor = the handle's
// current coupling, pmaf_fcouple.hpp; r = the staged list's radii):
//   term 0          the end effectors:                     d = xh_k - yh_k,                 R = separation
//   term 1 + s      src[a][s] == b (s ascending):           d = xh_k - z,  z = RN(anchor[a][s] + RN(scale[a][s] * yh_k)),
//                                                           R = RN(radius + r[a][s])
//   term 1 + M + s  src[b][s] == a (s ascending):           d = yh_k - z,  z = RN(anchor[b][s] + RN(scale[b][s] * xh_k)),
//                                                           R = RN(radius + r[b][s])
//   d2_t   = min over k of dot(d, d), strict `<` from +inf, k ascending (a NaN never wins)
//   gap_t  = sqrt(d2_t) - R_t                               (+inf when nothing won)
//   clearance = min over t of gap_t, strict `<` from +inf in term order: ties go to the smallest term, then the smallest
//   k; step = the winning term's k, sphere = its code t; +inf / -1 / -1 when nothing won or a path is empty.
//
// k_cross_audit_attached   the tile and the step walk of pmaf_cross_audit.hpp (ownership, LDS layout, staging, the hold
//                 rule, the prologue, xaudit_step_walk), terms outermost (pmaf_xattach_terms.hpp: the loop over the terms,
//                 the ride, the fold and the store, shared with k_xaudit_attached_slack).
//                  - a term's transform is applied AT STAGING: the tile of the path the sphere rides on is stored as z
//                    (XAttachRide through xaudit_stage_with: one multiply and one add per staged double, 6 flops per
//                    path point and term instead of 6 per pair-step); the other tile is staged as it lies. The step
//                    loop is then k_cross_audit's on the two staged tiles, d = a - b. For the terms 1 + M + s that is
//                    z - yh_k, the negation of the contract's d: every component's square, and so dot(d, d) in either
//                    association, has the same bits.
//                  - at the end of a term the thread folds (d2, k) of each of its 2 x 2 pairs into the pair's running
//                    (gap, k, t): one sqrt per pair and term, not per step; the strict `<` in term order is the tie rule.
//                  - steps past a pair's K: the step walk's remark (the ride of a held point is the held ride).
//                  - LDS is k_cross_audit's (two tiles of one chunk, 25.6 KB per block); no atomics, a pair belongs to
//                    one thread, the result does not depend on the grid.
//                  - with nothing attached the result is k_cross_audit's bit for bit (term 0 is its loop and its root).
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_cross_audit.hpp"
#include "pmaf_xattach.hpp"
#include "pmaf_xattach_terms.hpp"

using namespace pmaf;

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_cross_audit_attached(CrossAuditAttachedArgs S) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  __shared__ double s_a[C * 3 * TP], s_b[C * 3 * TP];
  __shared__ int s_na[T], s_nb[T], s_k[1];
  const CrossAuditArgs &A = S.X;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  const int K = xaudit_tile_lengths(A, a0, b0, s_na, s_nb, s_k);
  const double inf = __builtin_huge_val();
  XAttachBest p00, p01, p10, p11;   // the four pairs' running (gap, k, t): named, an array changed the kernel's code
  xattach_for_each_term(S, [&](int t, const XAttachRide fa, const XAttachRide fb, double R) {
    double best[2][2] = {{inf, inf}, {inf, inf}};
    int bk[2][2] = {{-1, -1}, {-1, -1}};
    xaudit_step_walk(A, a0, b0, K, s_a, s_b, s_na, s_nb, tx, ty, fa, fb, best, bk);
    p00.fold(best[0][0], bk[0][0], -1, R, t);
    p01.fold(best[0][1], bk[0][1], -1, R, t);
    p10.fold(best[1][0], bk[1][0], -1, R, t);
    p11.fold(best[1][1], bk[1][1], -1, R, t);
  });
  xattach_store_pair(S, a0, b0, ty, tx, s_na, s_nb, p00, nullptr);
  xattach_store_pair(S, a0, b0, ty, tx + 16, s_na, s_nb, p01, nullptr);
  xattach_store_pair(S, a0, b0, ty + 16, tx, s_na, s_nb, p10, nullptr);
  xattach_store_pair(S, a0, b0, ty + 16, tx + 16, s_na, s_nb, p11, nullptr);
}

void pmaf_k_launch_cross_audit_attached(const CrossAuditAttachedArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_cross_audit_attached, xaudit_grid(A.X), dim3(PMAF_XAUDIT_THREADS), 0, s, A);
}
