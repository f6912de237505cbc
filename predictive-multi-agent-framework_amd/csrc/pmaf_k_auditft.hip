// pmaf_k_auditft.hip -- the audits against the obstacle tracks (include/pmaf.h "audits against the obstacle tracks"):
// the kernels of pmaf_select_clear_tracked and pmaf_evaluate_paths_tracked that differ from the untracked calls', and
// their launchers. A translation unit of its own, object auditft.o: the code objects of the other units stay byte for
// byte what they were (NOTES.md 1: code placement alone moves the rollout loop).
//
// Semantics (the host-side contract is in include/pmaf.h). Everything is pmaf_select_clear's / pmaf_evaluate_paths'
// contract but the position of a tracked field obstacle: for population p with L = len[p] > 0 and f = min(first[p], L-1),
// obstacle j < M = n_obs - 1 at step k is at the POSITION of track point min(f + k, L-1), taken verbatim and held at the
// end (the rollout's rule, pmaf_ftrack.hpp; the track's velocities are not read). The trailing obstacle j = M, and every
// obstacle of a population with L == 0, stays on the list's iterated line o^{k+1} = o^k + RN(v dt). The radii are the
// caller's list's.
//
// k_ft_select_audit  k_select_audit's shape: one block of four waves per (agent, population), the four waves take the
//                    four quarters of the window, lane = obstacle. Tracks exist only on the one-slot route (<= 60 field
//                    obstacles), so n_obs <= 61: one tile, no j0 loop.
//                     - lanes j < M of a tracked population read the layout [P][max_len][6][64] (pmaf_ftrack.hpp): the
//                       point index is wave-uniform, the three position rows lie 0 / 512 / 1024 bytes from one lane
//                       pointer, each a contiguous row across the wave. Step k + 1's point is requested before step k's
//                       square root is taken, so the load's latency hides behind the ~50 operations of an audited step.
//                       No dependent chain, no k0 prefix walk. Columns >= M of the layout are zero and loaded harmlessly.
//                     - lane j = M walks the list's chain exactly as k_select_audit does (pre-rounded s = v dt, k0
//                       prefix adds, same order): its bits are the untracked kernel's. Every lane carries the chain's
//                       three adds (they are free beside the square root); only lane M's are consumed.
//                     - a population with L == 0 takes k_select_audit's loop as it is (block-uniform branch, no loads).
//                     - lanes >= n_audit are predicated off the minima, never clamped into another lane's column.
//                     - reductions as in k_select_audit: minima of doubles and integers, butterflies, then LDS across
//                       the waves. No atomics.
// k_audit_track_ft   k_audit_track's buffer [P][cap][3][n_obs]: one thread per (population, obstacle); a tracked column
//                    copies the positions of points min(f + k, L-1), the others run k_audit_track's chain. k_path_audit
//                    (pmaf_k_misc.hip) then runs unchanged on it.
// k_ft_masked_audit  k_ft_select_audit's body with the audited columns of two populations given as masks
//                    (pmaf_xattach.hpp: the joint selection on coupled handles leaves the columns that ride on the other
//                    member of the pair to its pair side); both kernels are instances of ft_select_audit<COLS>.
// The list is staged by k_select_stage and the pick is k_select_pick (pmaf_k_select.hip), both unchanged.
// (The name is k_ft_select_audit, not k_select_audit_ft: tests/test_select_clear.py and tests/test_pair_clear.py find
// k_select_audit's line of the resource record by substring and expect exactly one.)
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_auditft.hpp"
#include "pmaf_xattach.hpp"

using namespace pmaf;

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

// the body of both select audits. COLS: the audited columns are the bits of `cols` (k_ft_masked_audit) instead of the
// columns below n_audit
template <bool COLS>
__device__ __forceinline__ void ft_select_audit(const DevView &D, const SelectArgs &A, const FTrackArgs &F,
                                                unsigned long long cols) {
  __shared__ double s_c[PMAF_SELECT_WAVES];
  __shared__ int s_v[PMAF_SELECT_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pop = blockIdx.y, a = blockIdx.x;
  const int n_obs = D.n_obs;       // the lists' stride; <= 64 here (the launcher refuses more)
  const int M = n_obs - 1;
  const int n_audit = A.n_audit;   // n_obs, or n_obs - 1 (skip_trailing)
  PMAF_BOUND(n_obs >= 1 && n_obs <= 64 && n_audit >= 0 && n_audit <= n_obs);
  const size_t pa = (size_t)pop * D.N + a;
  int n = D.n_points[pa];
  PMAF_BOUND(n >= 0 && n <= D.cap);
  n = n < D.cap ? n : D.cap;
  PMAF_BOUND(A.horizon >= 1 && A.horizon <= D.cap);
  const int w = n < A.horizon ? n : A.horizon;
  const int chunk = (w + PMAF_SELECT_WAVES - 1) / PMAF_SELECT_WAVES;
  const int k0 = wave * chunk < w ? wave * chunk : w;
  const int k1 = k0 + chunk < w ? k0 + chunk : w;
  const double *path = D.paths + pa * (size_t)D.cap * 3;
  const double *o = A.obs + (size_t)pop * 7 * n_obs;
  const double dt = D.C.dt;
  const double inf = __builtin_huge_val();
  int L, f;
  ft_window(F, pop, L, f);

  double best = inf;
  int viol = 0x7fffffff;
  if (k0 < k1) {
    const int j = lane;
    const bool jv = COLS ? ((cols >> j) & 1ull) != 0 : j < n_audit;
    const int jc = j < n_obs ? j : 0;   // (the list's loads only; never a track column)
    V3 q = mk(o[jc], o[n_obs + jc], o[2 * (size_t)n_obs + jc]);
    // predictObstacles' v * dt, rounded once: the same double in every step of the chain
    const V3 s = mk(o[3 * (size_t)n_obs + jc] * dt, o[4 * (size_t)n_obs + jc] * dt, o[5 * (size_t)n_obs + jc] * dt);
    const double rr = D.C.rad + o[6 * (size_t)n_obs + jc];
    for (int k = 0; k < k0; k++) {   // the chain up to this wave's first step
      q.x = q.x + s.x;
      q.y = q.y + s.y;
      q.z = q.z + s.z;
    }
    if (L > 0) {   // block-uniform
      const bool tracked = lane < M;
      // this lane's column of the population's points; point i lies i * PMAF_FTRACK_POINT doubles further (wave-uniform)
      const double *col = F.pts + (size_t)pop * F.max_len * PMAF_FTRACK_POINT + lane;
      const int last = L - 1;
      int i = f + k0 < last ? f + k0 : last;
      const double *tp = col + (size_t)i * PMAF_FTRACK_POINT;
      V3 t = mk(tp[0], tp[PMAF_FTRACK_LANES], tp[2 * PMAF_FTRACK_LANES]);
      for (int k = k0; k < k1; k++) {
        // the next step's point (held at the end: always a point of the track, also behind the window's last step)
        i = f + k + 1 < last ? f + k + 1 : last;
        tp = col + (size_t)i * PMAF_FTRACK_POINT;
        const V3 tn = mk(tp[0], tp[PMAF_FTRACK_LANES], tp[2 * PMAF_FTRACK_LANES]);
        const V3 x = mk(path[k * 3], path[k * 3 + 1], path[k * 3 + 2]);
        const V3 ob = tracked ? t : q;
        const double c = norm(x - ob) - rr;
        if (jv) {
          if (c < best) best = c;
          if (c < A.margin && k < viol) viol = k;
        }
        q.x = q.x + s.x;
        q.y = q.y + s.y;
        q.z = q.z + s.z;
        t = tn;
      }
    } else {   // no tracks: k_select_audit's loop
      for (int k = k0; k < k1; k++) {
        const V3 x = mk(path[k * 3], path[k * 3 + 1], path[k * 3 + 2]);
        const double c = norm(x - q) - rr;
        if (jv) {
          if (c < best) best = c;
          if (c < A.margin && k < viol) viol = k;
        }
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

__global__ __launch_bounds__(64 * PMAF_SELECT_WAVES) void k_ft_select_audit(DevView D, SelectArgs A, FTrackArgs F) {
  ft_select_audit<false>(D, A, F, 0ull);
}

// the joint selection on a coupled handle (pmaf_select_pair_clear_tracked): the columns that ride on the OTHER member of
// the pair are left to the pair side. The two populations' audited columns come by value; every other population of the
// handle keeps the columns below n_audit. A mask is cut to the list (bits >= n_obs never count).
__global__ __launch_bounds__(64 * PMAF_SELECT_WAVES) void k_ft_masked_audit(DevView D, SelectArgs A, FTrackArgs F, AuditColumns C) {
  const int pop = blockIdx.y;
  const int n_obs = D.n_obs < 64 ? D.n_obs : 64;
  const unsigned long long list = n_obs >= 64 ? ~0ull : (1ull << n_obs) - 1ull;
  const int n_audit = A.n_audit < n_obs ? (A.n_audit > 0 ? A.n_audit : 0) : n_obs;
  unsigned long long cols = n_audit >= 64 ? ~0ull : (1ull << n_audit) - 1ull;
  cols = pop == C.pop_a ? C.cols_a : (pop == C.pop_b ? C.cols_b : cols);
  ft_select_audit<true>(D, A, F, cols & list);
}

__global__ __launch_bounds__(64) void k_audit_track_ft(int P, int n_obs, int cap, double dt, const double *obs /*[P][7][n_obs]*/,
                                                       FTrackArgs F, double *track /*[P][cap][3][n_obs]*/) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P * n_obs) return;
  const int pop = idx / n_obs, j = idx - pop * n_obs;
  int L, f;
  ft_window(F, pop, L, f);
  double *t = track + (size_t)pop * cap * 3 * n_obs + j;
  if (L > 0 && j < n_obs - 1) {
    PMAF_BOUND(j < PMAF_FTRACK_LANES);
    const double *col = F.pts + (size_t)pop * F.max_len * PMAF_FTRACK_POINT + j;
    const int last = L - 1;
    for (int k = 0; k < cap; k++) {
      const int i = f + k < last ? f + k : last;
      const double *tp = col + (size_t)i * PMAF_FTRACK_POINT;
      t[0] = tp[0]; t[n_obs] = tp[PMAF_FTRACK_LANES]; t[2 * (size_t)n_obs] = tp[2 * PMAF_FTRACK_LANES];
      t += 3 * (size_t)n_obs;
    }
    return;
  }
  const double *o = obs + (size_t)pop * 7 * n_obs;
  V3 q = mk(o[j], o[n_obs + j], o[2 * n_obs + j]);
  const V3 v = mk(o[3 * n_obs + j], o[4 * n_obs + j], o[5 * n_obs + j]);
  for (int k = 0; k < cap; k++) {
    t[0] = q.x; t[n_obs] = q.y; t[2 * (size_t)n_obs] = q.z;
    t += 3 * (size_t)n_obs;
    // predictObstacles, B/src/cf_agent.cpp:270-276
    q.x = q.x + v.x * dt;
    q.y = q.y + v.y * dt;
    q.z = q.z + v.z * dt;
  }
}

void pmaf_k_launch_select_audit_ft(const DevView &D, const SelectArgs &A, const FTrackArgs &F, hipStream_t s) {
  hipLaunchKernelGGL(k_ft_select_audit, dim3((unsigned)D.N, (unsigned)D.P), dim3(64 * PMAF_SELECT_WAVES), 0, s, D, A, F);
}

void pmaf_k_launch_masked_audit_ft(const DevView &D, const SelectArgs &A, const FTrackArgs &F, const AuditColumns &cols,
                                   hipStream_t s) {
  hipLaunchKernelGGL(k_ft_masked_audit, dim3((unsigned)D.N, (unsigned)D.P), dim3(64 * PMAF_SELECT_WAVES), 0, s, D, A, F, cols);
}

void pmaf_k_launch_audit_track_ft(const DevView &D, const double *obs, const FTrackArgs &F, double *track, hipStream_t s) {
  hipLaunchKernelGGL(k_audit_track_ft, dim3((D.P * D.n_obs + 63) / 64), dim3(64), 0, s, D.P, D.n_obs, D.cap, D.C.dt, obs, F, track);
}
