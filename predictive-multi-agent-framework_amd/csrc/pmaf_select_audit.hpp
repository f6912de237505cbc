// pmaf_select_audit.hpp -- select_audit_body<FT, COLS>: the ONE body of the selections' obstacle-side audit. Device code
// only (hipcc), no kernel of its own; its three instances keep their units and their names:
//   k_select_audit     <false, false>  pmaf_k_select.hip  (select.o)   pmaf_select_clear, the joint selection
//   k_ft_select_audit  <true,  false>  pmaf_k_auditft.hip (auditft.o)  the same calls on a handle with obstacle tracks
//   k_ft_masked_audit  <true,  true>   pmaf_k_auditft.hip (auditft.o)  the joint selection on coupled handles
//
// Semantics (the host-side contract is in include/pmaf.h). For agent (p, a) with n = n_points[p][a] the audit window is
// the first w = min(n, horizon) points of the current path; inside it everything is pmaf_evaluate_paths' contract:
//   o_j^0 = the caller's position, o_j^{k+1} = o_j^k + v_j * dt   (one multiply, one add per component, each rounded)
//   c(k, j) = norm(x_k - o_j^k) - (rad + r_j)                     (the build's dot association; no floor, no cap)
//   c_a  = min over k < w and audited j by a strict `<` from +inf (a NaN pair never wins), +inf for w = 0 or no audited j
//   fv_a = the smallest k < w with c(k, j) < margin for some audited j, else w;    clear_a <=> fv_a == w
// The audited obstacles are j < n_audit (n_obs, or n_obs - 1 when the joint selection leaves the trailing obstacle to the
// cross audit), or with COLS the bits of `cols` (pmaf_xattach.hpp: the columns that ride on the other member of the pair
// are left to its pair side).
// FT -- the position of a tracked field obstacle, all that differs: for population p with L = len[p] > 0 and
// f = min(first[p], L-1), obstacle j < M = n_obs - 1 at step k is at the POSITION of track point min(f + k, L-1), taken
// verbatim and held at the end (the rollout's rule, pmaf_ftrack.hpp; the track's velocities are not read). The trailing
// obstacle j = M, and every obstacle of a population with L == 0, stays on the list's iterated line. The radii are the
// caller's list's.
//
// Shape: one block of four waves per (agent, population); lane = obstacle j of a tile of 64; the four waves take the four
// quarters [q * ceil(w / 4), (q + 1) * ceil(w / 4)) of the window.
//  - the list's chain: the lane keeps its obstacle's position in three registers and advances it by the pre-rounded
//    s = v * dt, one add per component and step. v * dt is the same rounded product in every step of k_audit_track's
//    chain (-ffp-contract=off: the multiply and the add are never fused), so hoisting it changes no bit; and the chain
//    o^{k+1} = o^k + s is walked from o^0 in the same order, so o^k has k_audit_track's bits for every k. A wave that
//    starts at step k0 first walks the k0 adds of the chain alone (3 adds per step against ~50 operations of an audited
//    step).
//  - FT == false holds no track code and passes over the quarter once per obstacle tile (n_obs is unbounded there).
//  - FT == true: tracks exist only on the one-slot route (<= 60 field obstacles), so n_obs <= 64 (the host refuses more):
//    one tile. Lanes j < M of a tracked population read the layout [P][max_len][6][64] (pmaf_ftrack.hpp): the point index
//    is wave-uniform, the three position rows lie 0 / 512 / 1024 bytes from one lane pointer, each a contiguous row across
//    the wave. Step k + 1's point is requested before step k's square root is taken, so the load's latency hides behind
//    the audited step. No dependent chain for those lanes; columns >= M of the layout are zero and loaded harmlessly.
//    Every lane still carries the list chain's three adds (free beside the square root); only lane M's are consumed. A
//    population with L == 0 takes the untracked loop (block-uniform branch, no loads).
//  - lanes that are not audited are predicated off the minima, never clamped into another lane's column.
//  - the path point is a wave-uniform load; horizon bounds the loop (the caller's lever at tick rate).
//  - reductions are minima of doubles (no NaN ever enters one) and of integers: exact, associative and commutative, so
//    neither the split over waves nor the lane butterflies change a bit. No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_ftrack.hpp"

namespace pmaf {

#define PMAF_SELECT_WAVES 4

// the population's track length and clamped offset: L in [0, max_len], f in [0, L-1] (0 for L == 0)
__device__ __forceinline__ void ft_window(const FTrackArgs &F, int pop, int &L, int &f) {
  L = F.len ? F.len[pop] : 0;
  PMAF_BOUND(L >= 0 && L <= F.max_len);
  L = L < F.max_len ? L : F.max_len;
  L = L > 0 ? L : 0;
  f = L > 0 ? F.first[pop] : 0;
  PMAF_BOUND(f >= 0);
  f = f > 0 ? f : 0;
  f = f < L - 1 ? f : (L > 0 ? L - 1 : 0);   // clamped before any k is added: first may be INT32_MAX
}

// path point k against the obstacle at `ob` (rr = rad + r_j); jv: this lane's obstacle is audited
__device__ __forceinline__ void select_audit_step(const double *path, int k, const V3 &ob, double rr, bool jv, double margin,
                                                  double &best, int &viol) {
  const V3 x = mk(path[k * 3], path[k * 3 + 1], path[k * 3 + 2]);
  const double c = norm(x - ob) - rr;
  // (selects, not a block under jv: nothing for the compiler to sink the square root into)
  best = (jv && c < best) ? c : best;
  viol = (jv && c < margin && k < viol) ? k : viol;
}

template <bool FT, bool COLS>
__device__ __forceinline__ void select_audit_body(const DevView &D, const SelectArgs &A, const FTrackArgs &F,
                                                  unsigned long long cols) {
  static_assert(FT || !COLS, "column masks: the one-tile audit only");
  __shared__ double s_c[PMAF_SELECT_WAVES];
  __shared__ int s_v[PMAF_SELECT_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pop = blockIdx.y, a = blockIdx.x;
  const int n_obs = D.n_obs;       // the lists' stride
  const int n_audit = A.n_audit;   // the audited obstacles: n_obs, or n_obs - 1 (the joint selection skips the trailing one)
  PMAF_BOUND(n_audit >= 0 && n_audit <= n_obs && (!FT || (n_obs >= 1 && n_obs <= 64)));
  const size_t pa = (size_t)pop * D.N + a;
  int n = D.n_points[pa];
  PMAF_BOUND(n >= 0 && n <= D.cap);
  n = n < D.cap ? n : D.cap;
  PMAF_BOUND(A.horizon >= 1 && A.horizon <= D.cap);
  const int w = n < A.horizon ? n : A.horizon;
  // this wave's quarter of the window (block-uniform w, wave-uniform bounds)
  const int chunk = (w + PMAF_SELECT_WAVES - 1) / PMAF_SELECT_WAVES;
  const int k0 = wave * chunk < w ? wave * chunk : w;
  const int k1 = k0 + chunk < w ? k0 + chunk : w;
  const double *path = D.paths + pa * (size_t)D.cap * 3;
  const double *o = A.obs + (size_t)pop * 7 * n_obs;
  const double dt = D.C.dt;
  const double inf = __builtin_huge_val();
  int L = 0, f = 0;
  if constexpr (FT) ft_window(F, pop, L, f);

  double best = inf;
  int viol = 0x7fffffff;
  if (k0 < k1) {
    const int j_end = FT ? 1 : n_audit;   // FT: the one tile whatever n_audit says (a mask may audit beyond it)
    for (int j0 = 0; j0 < j_end; j0 += 64) {   // one pass over the quarter per obstacle tile
      const int j = j0 + lane;
      const bool jv = COLS ? ((cols >> j) & 1ull) != 0 : j < n_audit;
      const int jc = (COLS ? j < n_obs : jv) ? j : 0;   // (the list's loads only; never a track column)
      V3 q = mk(o[jc], o[n_obs + jc], o[2 * (size_t)n_obs + jc]);
      // predictObstacles' v * dt, rounded once: the same double in every step of the chain
      const V3 s = mk(o[3 * (size_t)n_obs + jc] * dt, o[4 * (size_t)n_obs + jc] * dt, o[5 * (size_t)n_obs + jc] * dt);
      const double rr = D.C.rad + o[6 * (size_t)n_obs + jc];
      for (int k = 0; k < k0; k++) {   // the chain up to this wave's first step
        q.x = q.x + s.x;
        q.y = q.y + s.y;
        q.z = q.z + s.z;
      }
      int k = k0;
      if constexpr (FT) {
        if (L > 0) {   // block-uniform
          const bool tracked = lane < n_obs - 1;
          // this lane's column of the population's points; point i lies i * PMAF_FTRACK_POINT doubles further (wave-uniform)
          const double *col = F.pts + (size_t)pop * F.max_len * PMAF_FTRACK_POINT + lane;
          const int last = L - 1;
          int i = f + k0 < last ? f + k0 : last;
          const double *tp = col + (size_t)i * PMAF_FTRACK_POINT;
          V3 t = mk(tp[0], tp[PMAF_FTRACK_LANES], tp[2 * PMAF_FTRACK_LANES]);
          for (; k < k1; k++) {
            // the next step's point (held at the end: always a point of the track, also behind the window's last step)
            i = f + k + 1 < last ? f + k + 1 : last;
            tp = col + (size_t)i * PMAF_FTRACK_POINT;
            const V3 tn = mk(tp[0], tp[PMAF_FTRACK_LANES], tp[2 * PMAF_FTRACK_LANES]);
            select_audit_step(path, k, tracked ? t : q, rr, jv, A.margin, best, viol);
            q.x = q.x + s.x;
            q.y = q.y + s.y;
            q.z = q.z + s.z;
            t = tn;
          }
        }
      }
      for (; k < k1; k++) {   // the untracked loop: every obstacle on the list's chain
        select_audit_step(path, k, q, rr, jv, A.margin, best, viol);
        q.x = q.x + s.x;
        q.y = q.y + s.y;
        q.z = q.z + s.z;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oc = __shfl_xor(best, off);
    const int ov = __shfl_xor(viol, off);
    best = (oc < best) ? oc : best;
    viol = (ov < viol) ? ov : viol;
  }
  if (lane == 0) { s_c[wave] = best; s_v[wave] = viol; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 1; q < PMAF_SELECT_WAVES; q++) {
      const double oc = s_c[q];
      const int ov = s_v[q];
      best = (oc < best) ? oc : best;
      viol = (ov < viol) ? ov : viol;
    }
    A.clr[pa] = best;
    A.fv[pa] = (viol == 0x7fffffff) ? w : viol;
  }
}

}  // namespace pmaf
