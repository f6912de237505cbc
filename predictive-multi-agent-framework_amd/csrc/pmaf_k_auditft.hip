// pmaf_k_auditft.hip -- the audits against the obstacle tracks (include/pmaf.h "audits against the obstacle tracks"):
// the kernels of pmaf_select_clear_tracked and pmaf_evaluate_paths_tracked that differ from the untracked calls', and
// their launchers. A translation unit of its own, object auditft.o: the code objects of the other units stay byte for
// byte what they were (NOTES.md 1: code placement alone moves the rollout loop).
//
// The select audit's contract and shape, tracked and untracked, are written down once, in pmaf_select_audit.hpp.
//
// k_ft_select_audit  select_audit_body<true, false>: k_select_audit with the field obstacles of a tracked population on
//                    their tracks.
// k_ft_masked_audit  select_audit_body<true, true>: the same with the audited columns of two populations given as masks
//                    (pmaf_xattach.hpp: the joint selection on coupled handles leaves the columns that ride on the other
//                    member of the pair to its pair side).
// k_audit_track_ft   k_audit_track's buffer [P][cap][3][n_obs]: one thread per (population, obstacle); a tracked column
//                    copies the positions of points min(f + k, L-1), the others run k_audit_track's chain
//                    (as audit_track_chain, pmaf_audit_chain.hpp). k_path_audit (pmaf_k_misc.hip) then runs unchanged on it.
// The list is staged by k_select_stage and the pick is k_select_pick (pmaf_k_select.hip), both unchanged.
// (The name is k_ft_select_audit, not k_select_audit_ft: tests/test_select_clear.py and tests/test_pair_clear.py find
// k_select_audit's line of the resource record by substring and expect exactly one.)
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_auditft.hpp"
#include "pmaf_xattach.hpp"
#include "pmaf_select_audit.hpp"
#include "pmaf_audit_chain.hpp"

using namespace pmaf;

__global__ __launch_bounds__(64 * PMAF_SELECT_WAVES) void k_ft_select_audit(DevView D, SelectArgs A, FTrackArgs F) {
  select_audit_body<true, false>(D, A, F, 0ull);
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
  select_audit_body<true, true>(D, A, F, cols & list);
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
  audit_track_chain(obs + (size_t)pop * 7 * n_obs, n_obs, j, cap, dt, t);
}

void pmaf_k_launch_select_audit_ft(const DevView &D, const SelectArgs &A, const FTrackArgs &F, const AuditColumns *cols,
                                   hipStream_t s) {
  const dim3 grid((unsigned)D.N, (unsigned)D.P), block(64 * PMAF_SELECT_WAVES);
  if (cols) hipLaunchKernelGGL(k_ft_masked_audit, grid, block, 0, s, D, A, F, *cols);
  else hipLaunchKernelGGL(k_ft_select_audit, grid, block, 0, s, D, A, F);
}

void pmaf_k_launch_audit_track_ft(const DevView &D, const double *obs, const FTrackArgs &F, double *track, hipStream_t s) {
  hipLaunchKernelGGL(k_audit_track_ft, dim3((D.P * D.n_obs + 63) / 64), dim3(64), 0, s, D.P, D.n_obs, D.cap, D.C.dt, obs, F, track);
}
