// pmaf_obstacle_slack.hpp -- the audits against the live list with timing slack (include/pmaf.h "clear selection with
// timing slack": pmaf_evaluate_paths_slack, pmaf_select_clear_slack): the launch interface between pmaf_host_audit.cpp and
// pmaf_k_obslack.hip, and -- for hipcc only -- obs_slack_audit_body<FT>, the one body of k_obs_slack_audit<false> (handles
// without obstacle tracks) and k_obs_slack_audit<true> (with). A header of its own so that no other kernel unit's inputs
// change with it: DevView, SelectArgs and FTrackArgs stay what they are.
//
// Semantics (the host-side contract is in include/pmaf.h). For agent (p, a) with n = n_points[p][a] the window is the
// first w = min(n, horizon) points of the current path. The obstacles have a time index l of their own; admitted are the
// pairs (k, l) with 0 <= k < w, l >= 0 and -early <= l - k <= late (late, early in [0, cap]: clamped on the host, so
// l < w + late <= 2 cap and no index overflows).
//   list obstacle:    o_j^0 = the caller's position, o_j^{l+1} = o_j^l + RN(v_j * dt): the chain of pmaf_select_audit.hpp,
//                     walked from o^0 and never multiplied out, so o^l has k_audit_track's bits for every l
//   tracked obstacle: (FT, a population with L = len[p] > 0, j < M = n_obs - 1) the POSITION of track point
//                     min(min(f, L-1) + l, L-1), verbatim and held at the end; the trailing obstacle j = M, and every
//                     obstacle of a population with L == 0, stays on the list's chain
//   c(k, l, j) = norm(x_k - o_j^l) - (rad + r_j)     (the build's dot association; radii from the caller's list)
//   c_a  = the minimum over admitted (k, l) and audited j < n_audit under the total order (c, k, l, j); a NaN or +inf
//          never wins; +inf with (step, obstacle_step, obstacle) = (-1, -1, -1) when nothing won
//   fv_a = the smallest k < w with c(k, l, j) < margin for some admitted l and audited j, else w: the ARM's step
// (late, early) = (0, 0) admits l == k only: k_select_audit's / k_ft_select_audit's clr and fv, and k_path_audit's
// (step, obstacle) with obstacle_step == step, bit for bit.
//
// Shape, from select_audit_body: one block of four waves per (agent, population); lane = obstacle j of a tile of 64
// (FT == false: any number of tiles; FT == true: one tile, n_obs <= 64, the host refuses more).
//  - l is the OUTER loop: the four waves take the quarters of [0, w + late). A wave that starts at l0 first walks the l0
//    adds of the chain alone. Each obstacle position is then produced once per wave -- three chain adds, or three
//    row loads of the layout [P][max_len][6][64] (pmaf_ftrack.hpp) with index l + 1's point requested before index l's
//    square roots -- and held against the at most late + early + 1 path points k in [l - late, l + early] n [0, w).
//  - the path point is a wave-uniform load. With the wave's number taken through readfirstlane, l, the band's bounds
//    and k are uniform for the compiler too, and the disassembly shows what that buys: the loops branch on SCC instead
//    of on the exec mask, and a path point is one s_load_dwordx4 + one s_load_dwordx2 from the scalar cache instead of
//    a global_load pair per lane with a vmcnt(0) in front of every pair. The source asks for point k + 1 (and the next
//    index's first point) ahead of point k's arithmetic; the compiler reuses the point's scalar registers and so issues
//    the request inside pair k's square-root refinement, some twenty instructions ahead of the wait (read off the
//    disassembly; whether that hides the scalar cache's latency, and that the loop is bound by its vector side, is
//    reasoned from the instruction mix, not measured). Staging the wave's slice of the path with its halo in LDS would put
//    three ds_read_b64 per pair on the vector side, which is the side this loop is bound by (~15 FP64 operations and
//    the correctly rounded square root per pair); the scalar loads cost the vector side nothing.
//  - this traversal is not (k, l)-ascending, so the per-lane best keeps (c, k, l) and is replaced on c < best or on an
//    equal c with a smaller (k, l); a lane's j grows with the tile, so an equal (c, k, l) keeps the earlier tile's j. The
//    lane butterflies and the four-wave fold compare (c, k, l, j): minima under a total order, exact and independent of
//    the split. first_violation is an integer minimum.
//  - lanes that are not audited are predicated off the minima, never clamped into another lane's column.
//  - no atomics, no scratch, 96 bytes of LDS for the fold.
#pragma once
#include "pmaf_types.hpp"
#include "pmaf_ftrack.hpp"

struct ObsSlackArgs {
  const double *obs;        // [P][7][n_obs] SoA on the device: the caller's live list, already staged
  double margin;
  int horizon;              // 1 .. cap (clamped on the host)
  int n_audit;              // obstacles 0 .. n_audit - 1 of every list are audited: n_obs, or n_obs - 1 (skip_trailing)
  int late, early;          // 0 .. cap each (clamped on the host)
  double *clr;              // [P][N] c_a   (the selection: SelectArgs::clr)
  int32_t *fv;              // [P][N] fv_a  (the selection: SelectArgs::fv)
  int32_t *step, *obstacle_step, *obstacle;   // [P][N] each, or NULL (the selection reads none of them)
};

// pmaf_k_obslack.hip: k_obs_slack_audit<false> on grid (N, P), or with F != NULL k_obs_slack_audit<true> (needs
// D.n_obs <= 64; a tracked handle has <= 61)
void pmaf_k_launch_obs_slack_audit(const DevView &D, const ObsSlackArgs &A, const FTrackArgs *F, hipStream_t s);

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "pmaf_device.hpp"
#include "pmaf_select_audit.hpp"   // PMAF_SELECT_WAVES, ft_window

namespace pmaf {

__device__ __forceinline__ V3 obs_slack_point(const double *path, int k) {
  return mk(path[k * 3], path[k * 3 + 1], path[k * 3 + 2]);
}
// the first path point of index l's band, cut to the window (always a point of the path: w > 0 here)
__device__ __forceinline__ int obs_slack_lo(int l, int late, int w) {
  const int lo = l - late > 0 ? l - late : 0;
  return lo < w - 1 ? lo : w - 1;
}

// the per-lane best under (c, k, l): the obstacle at index l against path points lo .. hi (wave-uniform bounds); x = path
// point lo, already requested by the caller. Point k + 1 is requested while point k is worked on (held at hi).
__device__ __forceinline__ void obs_slack_points(const double *path, int lo, int hi, int l, V3 x, const V3 &ob, double rr,
                                                 bool jv, int j, double margin, double &bc, int &bk, int &bl, int &bj,
                                                 int &viol) {
  const double inf = __builtin_huge_val();
  for (int k = lo; k <= hi; k++) {
    const V3 xn = obs_slack_point(path, k < hi ? k + 1 : hi);
    const double c = norm(x - ob) - rr;
    // (selects on bitwise conditions, not a block under jv: nothing for the compiler to branch on or to sink the square
    // root into)
    const bool take = jv & ((c < bc) | ((c == bc) & (c < inf) & ((k < bk) | ((k == bk) & (l < bl)))));
    bc = take ? c : bc;
    bk = take ? k : bk;
    bl = take ? l : bl;
    bj = take ? j : bj;
    viol = (jv & (c < margin) & (k < viol)) ? k : viol;
    x = xn;
  }
}

// (c, k, l, j) of `o` before that of the running best; kl = k << 32 | l
__device__ __forceinline__ bool obs_slack_before(double oc, unsigned long long okl, int oj, double c, unsigned long long kl,
                                                 int j) {
  return oc < c || (oc == c && (okl < kl || (okl == kl && oj < j)));
}

template <bool FT>
__device__ __forceinline__ void obs_slack_audit_body(const DevView &D, const ObsSlackArgs &A, const FTrackArgs &F) {
  __shared__ double s_c[PMAF_SELECT_WAVES];
  __shared__ unsigned long long s_kl[PMAF_SELECT_WAVES];
  __shared__ int s_j[PMAF_SELECT_WAVES], s_v[PMAF_SELECT_WAVES];
  // (the wave's number in a scalar register: l, the band's bounds and k are then wave-uniform for the compiler as well)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int pop = blockIdx.y, a = blockIdx.x;
  const int n_obs = D.n_obs;       // the lists' stride
  const int n_audit = A.n_audit;
  PMAF_BOUND(n_audit >= 0 && n_audit <= n_obs && (!FT || (n_obs >= 1 && n_obs <= 64)));
  const size_t pa = (size_t)pop * D.N + a;
  int n = D.n_points[pa];
  PMAF_BOUND(n >= 0 && n <= D.cap);
  n = n < D.cap ? n : D.cap;
  PMAF_BOUND(A.horizon >= 1 && A.horizon <= D.cap);
  PMAF_BOUND(A.late >= 0 && A.late <= D.cap && A.early >= 0 && A.early <= D.cap);
  const int w = n < A.horizon ? n : A.horizon;
  const int late = A.late, early = A.early;
  // the obstacles' indices that meet the window: [0, w + late), none for an empty window; this wave's quarter of them
  const int span = w > 0 ? w + late : 0;
  const int chunk = (span + PMAF_SELECT_WAVES - 1) / PMAF_SELECT_WAVES;
  const int l0 = wave * chunk < span ? wave * chunk : span;
  const int l1 = l0 + chunk < span ? l0 + chunk : span;
  const double *path = D.paths + pa * (size_t)D.cap * 3;
  const double *o = A.obs + (size_t)pop * 7 * n_obs;
  const double dt = D.C.dt;
  const double inf = __builtin_huge_val();
  int L = 0, f = 0;
  if constexpr (FT) ft_window(F, pop, L, f);

  double bc = inf;
  int bk = 0x7fffffff, bl = 0x7fffffff, bj = 0x7fffffff, viol = 0x7fffffff;
  if (l0 < l1) {
    const int j_end = FT ? (n_audit < 64 ? n_audit : 64) : n_audit;   // FT: the one tile
    for (int j0 = 0; j0 < j_end; j0 += 64) {   // one pass over the quarter per obstacle tile
      const int j = j0 + lane;
      const bool jv = j < n_audit;
      const int jc = jv ? j : 0;   // (the list's loads only; never a track column)
      V3 q = mk(o[jc], o[n_obs + jc], o[2 * (size_t)n_obs + jc]);
      // predictObstacles' v * dt, rounded once: the same double in every step of the chain
      const V3 s = mk(o[3 * (size_t)n_obs + jc] * dt, o[4 * (size_t)n_obs + jc] * dt, o[5 * (size_t)n_obs + jc] * dt);
      const double rr = D.C.rad + o[6 * (size_t)n_obs + jc];
      for (int l = 0; l < l0; l++) {   // the chain up to this wave's first index
        q.x = q.x + s.x;
        q.y = q.y + s.y;
        q.z = q.z + s.z;
      }
      int l = l0;
      V3 x0 = obs_slack_point(path, obs_slack_lo(l0, late, w));
      if constexpr (FT) {
        if (L > 0) {   // block-uniform
          const bool tracked = lane < n_obs - 1;
          // this lane's column of the population's points; point i lies i * PMAF_FTRACK_POINT doubles further (wave-uniform)
          const double *col = F.pts + (size_t)pop * F.max_len * PMAF_FTRACK_POINT + lane;
          const int last = L - 1;
          int i = f + l0 < last ? f + l0 : last;   // (f <= L - 1 and l < 2 cap: no overflow)
          const double *tp = col + (size_t)i * PMAF_FTRACK_POINT;
          V3 t = mk(tp[0], tp[PMAF_FTRACK_LANES], tp[2 * PMAF_FTRACK_LANES]);
          for (; l < l1; l++) {
            // the next index's point (held at the end: always a point of the track)
            i = f + l + 1 < last ? f + l + 1 : last;
            tp = col + (size_t)i * PMAF_FTRACK_POINT;
            const V3 tn = mk(tp[0], tp[PMAF_FTRACK_LANES], tp[2 * PMAF_FTRACK_LANES]);
            const int lo = obs_slack_lo(l, late, w);
            const int hi = l + early < w - 1 ? l + early : w - 1;
            const V3 x0n = obs_slack_point(path, obs_slack_lo(l + 1, late, w));   // the next index's first path point
            obs_slack_points(path, lo, hi, l, x0, tracked ? t : q, rr, jv, j, A.margin, bc, bk, bl, bj, viol);
            x0 = x0n;
            q.x = q.x + s.x;
            q.y = q.y + s.y;
            q.z = q.z + s.z;
            t = tn;
          }
        }
      }
      for (; l < l1; l++) {   // the untracked loop: every obstacle on the list's chain
        const int lo = obs_slack_lo(l, late, w);
        const int hi = l + early < w - 1 ? l + early : w - 1;
        const V3 x0n = obs_slack_point(path, obs_slack_lo(l + 1, late, w));
        obs_slack_points(path, lo, hi, l, x0, q, rr, jv, j, A.margin, bc, bk, bl, bj, viol);
        x0 = x0n;
        q.x = q.x + s.x;
        q.y = q.y + s.y;
        q.z = q.z + s.z;
      }
    }
  }
  unsigned long long kl = ((unsigned long long)(unsigned)bk << 32) | (unsigned)bl;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oc = __shfl_xor(bc, off);
    const unsigned long long okl = __shfl_xor(kl, off);
    const int oj = __shfl_xor(bj, off);
    const int ov = __shfl_xor(viol, off);
    const bool take = obs_slack_before(oc, okl, oj, bc, kl, bj);
    bc = take ? oc : bc;
    kl = take ? okl : kl;
    bj = take ? oj : bj;
    viol = (ov < viol) ? ov : viol;
  }
  if (lane == 0) { s_c[wave] = bc; s_kl[wave] = kl; s_j[wave] = bj; s_v[wave] = viol; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 1; q < PMAF_SELECT_WAVES; q++) {
      const double oc = s_c[q];
      const unsigned long long okl = s_kl[q];
      const int oj = s_j[q], ov = s_v[q];
      const bool take = obs_slack_before(oc, okl, oj, bc, kl, bj);
      bc = take ? oc : bc;
      kl = take ? okl : kl;
      bj = take ? oj : bj;
      viol = (ov < viol) ? ov : viol;
    }
    const bool found = bj != 0x7fffffff;
    A.clr[pa] = bc;
    A.fv[pa] = (viol == 0x7fffffff) ? w : viol;
    if (A.step) A.step[pa] = found ? (int)(kl >> 32) : -1;
    if (A.obstacle_step) A.obstacle_step[pa] = found ? (int)(kl & 0xffffffffull) : -1;
    if (A.obstacle) A.obstacle[pa] = found ? bj : -1;
  }
}

}  // namespace pmaf
#endif  // __HIPCC__
