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
// k_xaudit_attached_slack   the tile of pmaf_cross_audit.hpp (ownership, LDS layout, staging, the hold rule, the
//                 prologue), terms outermost as in k_cross_audit_attached, k_cross_audit_slack's walk inside a term.
//                  - terms: a block-uniform loop over the 2 M candidate columns; a term's parameters (side, scale,
//                    anchor, R) are read through uniform addresses from the coupling's resident rows and the staged
//                    list's radii and kept as VALUES (pmaf_k_xattach.hip: a conditional over struct members was
//                    indexed in scratch). Nothing is uploaded for a call beyond the list.
//                  - inside a term: for every chunk [k0, k0 + C) of A the block walks the chunks of B, on the grid of
//                    multiples of C, that meet the band [k0 - late_b, k0 + C - 1 + late_a] clipped to [0, K). A chunk
//                    pair inside the band runs the full C x C loop; at the two edge diagonals the band is the l loop's
//                    BOUNDS (k, l0 and the slacks are block-uniform: no lane mask).
//                  - the ride is applied AT STAGING (xaudit_stage_with): to A's chunk for a term 1 + M + s, to every
//                    chunk of B for a term 1 + s. A's chunk is therefore transformed once per term and k0, B's once
//                    per chunk PAIR (a chunk of B is restaged for every chunk of A that meets it, as in
//                    k_cross_audit_slack: 6 flops per staged double against up to 4 C^2 pair-steps per thread).
//                    The step loop is d = a - b on the two staged tiles. For the terms 1 + M + s that is z - yh_l, the
//                    negation of the contract's d: every component's square, and so dot(d, d) in either association,
//                    has the same bits.
//                  - tie rule inside a term: k_cross_audit_slack's. The traversal (chunk of A, chunk of B, k, l) visits
//                    a smaller (k, l) later iff its k is smaller, so
//                        take = (d2 < best) | ((d2 == best) & (k < best_k))
//                    keeps the least visited step under (d2, k, l); false for a NaN, false against (+inf, -1, -1).
//                  - at the end of a term the thread folds (d2, k, l) of each of its 2 x 2 pairs into the pair's running
//                    (gap, k, l, t): one sqrt per pair and term; the strict `<` in term order is the tie rule across
//                    terms. A term in which nothing won (every d2 NaN) has k = -1 and is not folded.
//                  - steps past a pair's own K = max(n, m) are visited where a longer neighbour of the tile (or the
//                    ragged last chunk) makes the block walk further. Such a step (k, l), max(k, l) >= K, cannot win a
//                    term: let k' = min(k, K - 1), l' = min(l, K - 1). Both paths have ended by K - 1, so xh_k' = xh_k
//                    and yh_l' = yh_l, and the ride of a held point is the held ride (the same multiply and add on the
//                    same bits): the term's d2(k', l') has the same bits. (k', l') is admitted: both clipped gives
//                    (K - 1, K - 1); only k clipped gives l - k' <= 0 <= late_a and l - k' > l - k >= -late_b; only l
//                    clipped the mirror image. And (k', l') < (k, l). So every such step ties with (or, NaN, loses
//                    like) an ADMITTED step of a smaller (k, l) that the block also visits in the same term, and the
//                    order above never prefers it.
//                  - LDS: two tiles of one chunk plus the lengths, 25 608 B per block, independent of the slack and of
//                    the number of terms; no atomics, a pair belongs to one thread, the result does not depend on the
//                    grid.
//                  - xslack_row is restated here (not moved into pmaf_cross_audit.hpp): slack.o's inputs stay what they
//                    were.
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_cross_audit.hpp"
#include "pmaf_xattach.hpp"

using namespace pmaf;

// what is staged of a path point (k_cross_audit_attached's functor, restated: that unit's object does not change). on:
// the sphere that rides on it -- one rounded multiply, one rounded add per component (the composer's formula; this unit
// is compiled without contraction); otherwise the point as it lies. `on` is block-uniform.
struct XAttachSlackRide {
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

// the two points of B at staged row l against the two of A in registers: 4 pair-steps (k_cross_audit_slack's row)
__device__ __forceinline__ void xattach_slack_row(const V3 (&x)[2], const double *rb, int kk, int ll, double (&best)[2][2],
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
      const bool take = (d2 < best[r][c]) | ((d2 == best[r][c]) & (kk < bk[r][c]));
      best[r][c] = take ? d2 : best[r][c];
      bk[r][c] = take ? kk : bk[r][c];
      bl[r][c] = take ? ll : bl[r][c];
    }
}

__global__ __launch_bounds__(PMAF_XAUDIT_THREADS) void k_xaudit_attached_slack(CrossAuditAttachedSlackArgs S) {
  constexpr int T = PMAF_XAUDIT_TILE, C = PMAF_XAUDIT_CHUNK, TP = T + 1;
  __shared__ double s_a[C * 3 * TP], s_b[C * 3 * TP];
  __shared__ int s_na[T], s_nb[T], s_k[1];
  const CrossAuditArgs &A = S.T.X;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  const int late_a = S.late_a, late_b = S.late_b;
  const int K = xaudit_tile_lengths(A, a0, b0, s_na, s_nb, s_k);
  const int M = S.T.M;
  PMAF_BOUND(M >= 0 && ((!S.T.a.src && !S.T.b.src) || M <= PMAF_FTRACK_LANES));
  PMAF_BOUND(late_a >= 0 && late_a <= A.cap && late_b >= 0 && late_b <= A.cap);
  const double inf = __builtin_huge_val();
  // the four pairs' running (gap, k, l, t)
  double gap00 = inf, gap01 = inf, gap10 = inf, gap11 = inf;
  int gk00 = -1, gk01 = -1, gk10 = -1, gk11 = -1, gl00 = -1, gl01 = -1, gl10 = -1, gl11 = -1;
  int gt00 = -1, gt01 = -1, gt10 = -1, gt11 = -1;
  const int n_terms = 1 + ((S.T.a.src || S.T.b.src) ? 2 * M : 0);
  for (int t = 0; t < n_terms; t++) {   // block-uniform, as is every branch on t below
    // which tile carries the sphere: neither (term 0), B's (a column of A's list rides on y) or A's
    bool on_a = false, on_b = false;
    double scale = 0.0, ax = 0.0, ay = 0.0, az = 0.0, R = A.separation;
    if (t > 0) {
      const bool of_a = t <= M;
      const int s = of_a ? t - 1 : t - 1 - M;
      const int32_t *src = of_a ? S.T.a.src : S.T.b.src;
      if (!src || src[s] != (of_a ? S.T.pop_b : S.T.pop_a)) continue;
      const double *anchor = of_a ? S.T.a.anchor : S.T.b.anchor;
      scale = (of_a ? S.T.a.scale : S.T.b.scale)[s];
      ax = anchor[s];
      ay = anchor[PMAF_FTRACK_LANES + s];
      az = anchor[2 * PMAF_FTRACK_LANES + s];
      on_b = of_a;
      on_a = !of_a;
      R = S.T.radius + (of_a ? S.T.a.rad : S.T.b.rad)[s];
    }
    const XAttachSlackRide fa{on_a, scale, ax, ay, az}, fb{on_b, scale, ax, ay, az};
    double best[2][2] = {{inf, inf}, {inf, inf}};
    int bk[2][2] = {{-1, -1}, {-1, -1}}, bl[2][2] = {{-1, -1}, {-1, -1}};
    for (int k0 = 0; k0 < K; k0 += C) {   // every trip count below is block-uniform
      xaudit_stage_with(s_a, A.paths_a, s_na, a0, A.n_a, A.cap, k0, fa);
      // the steps of B this chunk of A can meet, and the chunks (multiples of C) that hold them: lo <= k0 <= hi, so
      // the loop below runs at least once and its barriers order this chunk of A too
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
            for (int l = 0; l < C; l++) xattach_slack_row(x, s_b + l * 3 * TP + tx, k0 + k, l0 + l, best, bk, bl);
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
            for (int ll = l_lo; ll <= l_hi; ll++) xattach_slack_row(x, s_b + (ll - l0) * 3 * TP + tx, kk, ll, best, bk, bl);
          }
        }
        __syncthreads();
      }
    }
    // the term into the pair's running minimum: strict, terms ascending -- ties keep the smallest term
    const auto fold = [&](double d2, int k, int l, double &gap, int &gk, int &gl, int &gt) {
      const double g = __builtin_sqrt(d2) - R;
      const bool take = k >= 0 && g < gap;
      gap = take ? g : gap;
      gk = take ? k : gk;
      gl = take ? l : gl;
      gt = take ? t : gt;
    };
    fold(best[0][0], bk[0][0], bl[0][0], gap00, gk00, gl00, gt00);
    fold(best[0][1], bk[0][1], bl[0][1], gap01, gk01, gl01, gt01);
    fold(best[1][0], bk[1][0], bl[1][0], gap10, gk10, gl10, gt10);
    fold(best[1][1], bk[1][1], bl[1][1], gap11, gk11, gl11, gt11);
  }
  // the store: xaudit_store_pair's conventions (the ragged edge is not stored; an empty path on either side, or nothing
  // won: +inf / -1 / -1 / -1), on a gap that already has its root taken
  const auto store = [&](int r, int c, double gap, int gk, int gl, int gt) {
    const int ti = ty + 16 * r, tj = tx + 16 * c;
    const int i = a0 + ti, j = b0 + tj;
    if (i < A.n_a && j < A.n_b) {
      const bool won = gk >= 0 && s_na[ti] > 0 && s_nb[tj] > 0;
      const size_t o = (size_t)i * A.n_b + j;
      A.clearance[o] = won ? gap : inf;
      if (A.step) A.step[o] = won ? gk : -1;
      if (S.step_b) S.step_b[o] = won ? gl : -1;
      if (S.T.sphere) S.T.sphere[o] = won ? gt : -1;
    }
  };
  store(0, 0, gap00, gk00, gl00, gt00);
  store(0, 1, gap01, gk01, gl01, gt01);
  store(1, 0, gap10, gk10, gl10, gt10);
  store(1, 1, gap11, gk11, gl11, gt11);
}

void pmaf_k_launch_cross_audit_attached_slack(const CrossAuditAttachedSlackArgs &A, hipStream_t s) {
  const dim3 grid((unsigned)((A.T.X.n_b + PMAF_XAUDIT_TILE - 1) / PMAF_XAUDIT_TILE),
                  (unsigned)((A.T.X.n_a + PMAF_XAUDIT_TILE - 1) / PMAF_XAUDIT_TILE));
  hipLaunchKernelGGL(k_xaudit_attached_slack, grid, dim3(PMAF_XAUDIT_THREADS), 0, s, A);
}
