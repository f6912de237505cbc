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
// k_cross_audit_attached   the tile of pmaf_cross_audit.hpp (ownership, LDS layout, staging, the hold rule, the prologue:
//                 shared with k_cross_audit and k_cross_audit_slack), terms outermost.
//                  - a term's transform is applied AT STAGING: the tile of the path the sphere rides on is stored as z
//                    (xaudit_stage_with: one multiply and one add per staged double, 6 flops per path point and term
//                    instead of 6 per pair-step); the other tile is staged as it lies. The step loop is then
//                    k_cross_audit's on the two staged tiles, d = a - b. For the terms 1 + M + s that is z - yh_k, the
//                    negation of the contract's d: every component's square, and so dot(d, d) in either association,
//                    has the same bits.
//                  - a term's parameters (side, scale, anchor, R) are wave-uniform: read through uniform addresses from
//                    the coupling's rows; the walk over the 2 M candidate columns is a block-uniform loop of integer
//                    compares, and a handle without attachments runs term 0 alone.
//                  - at the end of a term the thread folds (d2, k) of each of its 2 x 2 pairs into the pair's running
//                    (gap, k, t): one sqrt per pair and term, not per step; the strict `<` in term order is the tie rule.
//                    A term in which nothing won (every d2 NaN) has k = -1 and is not folded.
//                  - steps past a pair's K and past the ragged end of the last chunk repeat a held point in BOTH tiles
//                    (the transform of a held point is the held transform), tie with an earlier step and never win.
//                  - LDS is k_cross_audit's (two tiles of one chunk, 25.6 KB per block); no atomics, a pair belongs to
//                    one thread, the result does not depend on the grid.
//                  - with nothing attached the result is k_cross_audit's bit for bit (term 0 is its loop and its root).
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_cross_audit.hpp"
#include "pmaf_xattach.hpp"

using namespace pmaf;

// what is staged of a path point. on: the sphere that rides on it -- one rounded multiply, one rounded add per component
// (the composer's formula, pmaf_k_fcouple.hip; this unit is compiled without contraction); otherwise the point as it
// lies. `on` is block-uniform.
struct XAttachRide {
  bool on;
  double scale, ax, ay, az;
  __device__ __forceinline__ double operator()(double v, int c) const {
    if (!on) return v;
    const double a0 = ax, a1 = ay, a2 = az;   // (values, not lvalues: the choice below must not become an address)
    const double a = c == 0 ? a0 : (c == 1 ? a1 : a2);
    const double m = scale * v;
    return a + m;
  }
};

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_cross_audit_attached(CrossAuditAttachedArgs S) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  __shared__ double s_a[C * 3 * TP], s_b[C * 3 * TP];
  __shared__ int s_na[T], s_nb[T], s_k[1];
  const CrossAuditArgs &A = S.X;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  const int K = xaudit_tile_lengths(A, a0, b0, s_na, s_nb, s_k);
  const int M = S.M;
  PMAF_BOUND(M >= 0 && ((!S.a.src && !S.b.src) || M <= PMAF_FTRACK_LANES));
  const double inf = __builtin_huge_val();
  // the four pairs' running (gap, k, t)
  double gap00 = inf, gap01 = inf, gap10 = inf, gap11 = inf;
  int gk00 = -1, gk01 = -1, gk10 = -1, gk11 = -1, gt00 = -1, gt01 = -1, gt10 = -1, gt11 = -1;
  const int n_terms = 1 + ((S.a.src || S.b.src) ? 2 * M : 0);
  for (int t = 0; t < n_terms; t++) {   // block-uniform, as is every branch on t below
    // which tile carries the sphere: neither (term 0), B's (a column of A's list rides on y) or A's
    bool on_a = false, on_b = false;
    double scale = 0.0, ax = 0.0, ay = 0.0, az = 0.0, R = A.separation;
    if (t > 0) {
      const bool of_a = t <= M;
      const int s = of_a ? t - 1 : t - 1 - M;
      const int32_t *src = of_a ? S.a.src : S.b.src;
      if (!src || src[s] != (of_a ? S.pop_b : S.pop_a)) continue;
      const double *anchor = of_a ? S.a.anchor : S.b.anchor;
      scale = (of_a ? S.a.scale : S.b.scale)[s];
      ax = anchor[s];
      ay = anchor[PMAF_FTRACK_LANES + s];
      az = anchor[2 * PMAF_FTRACK_LANES + s];
      on_b = of_a;
      on_a = !of_a;
      R = S.radius + (of_a ? S.a.rad : S.b.rad)[s];
    }
    const XAttachRide fa{on_a, scale, ax, ay, az}, fb{on_b, scale, ax, ay, az};
    double best[2][2] = {{inf, inf}, {inf, inf}};
    int bk[2][2] = {{-1, -1}, {-1, -1}};
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
    // the term into the pair's running minimum: strict, terms ascending -- ties keep the smallest term
    const auto fold = [&](double d2, int k, double &gap, int &gk, int &gt) {
      const double g = __builtin_sqrt(d2) - R;
      const bool take = k >= 0 && g < gap;
      gap = take ? g : gap;
      gk = take ? k : gk;
      gt = take ? t : gt;
    };
    fold(best[0][0], bk[0][0], gap00, gk00, gt00);
    fold(best[0][1], bk[0][1], gap01, gk01, gt01);
    fold(best[1][0], bk[1][0], gap10, gk10, gt10);
    fold(best[1][1], bk[1][1], gap11, gk11, gt11);
  }
  // the store: xaudit_store_pair's conventions (the ragged edge is not stored; an empty path on either side, or nothing
  // won: +inf / -1 / -1), on a gap that already has its root taken
  const auto store = [&](int r, int c, double gap, int gk, int gt) {
    const int ti = ty + 16 * r, tj = tx + 16 * c;
    const int i = a0 + ti, j = b0 + tj;
    if (i < A.n_a && j < A.n_b) {
      const bool won = gk >= 0 && s_na[ti] > 0 && s_nb[tj] > 0;
      const size_t o = (size_t)i * A.n_b + j;
      A.clearance[o] = won ? gap : inf;
      if (A.step) A.step[o] = won ? gk : -1;
      if (S.sphere) S.sphere[o] = won ? gt : -1;
    }
  };
  store(0, 0, gap00, gk00, gt00);
  store(0, 1, gap01, gk01, gt01);
  store(1, 0, gap10, gk10, gt10);
  store(1, 1, gap11, gk11, gt11);
}

void pmaf_k_launch_cross_audit_attached(const CrossAuditAttachedArgs &A, hipStream_t s) {
  const dim3 grid((unsigned)((A.X.n_b + PMAF_XAUDIT_TILE - 1) / PMAF_XAUDIT_TILE),
                  (unsigned)((A.X.n_a + PMAF_XAUDIT_TILE - 1) / PMAF_XAUDIT_TILE));
  hipLaunchKernelGGL(k_cross_audit_attached, grid, dim3(PMAF_XAUDIT_THREADS), 0, s, A);
}
