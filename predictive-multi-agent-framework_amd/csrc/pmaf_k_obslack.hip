// pmaf_k_obslack.hip -- the audits against the live list with timing slack (include/pmaf.h "clear selection with timing
// slack"): the kernel of pmaf_evaluate_paths_slack and pmaf_select_clear_slack, and its launcher. A translation unit of
// its own, object obslack.o (outside the k_*.o set of twelve): the code objects of the other units stay byte for byte
// what they were (NOTES.md 1: code placement alone moves the rollout loop).
//
// The contract and the shape are written down once, in pmaf_obstacle_slack.hpp.
//
// k_obs_slack_audit<false>  a handle without obstacle tracks: every obstacle on the list's chain, any number of tiles
// k_obs_slack_audit<true>   a handle with tracks: the field obstacles of a tracked population on their tracks, one tile
// The list is staged by the caller (k_select_stage for the selection, the path audit's upload for the evaluation); the
// selection's pick is k_select_pick (pmaf_k_select.hip) on the clr / fv this kernel leaves, unchanged.
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_obstacle_slack.hpp"

using namespace pmaf;

template <bool FT>
__global__ __launch_bounds__(64 * PMAF_SELECT_WAVES) void k_obs_slack_audit(DevView D, ObsSlackArgs A, FTrackArgs F) {
  obs_slack_audit_body<FT>(D, A, F);
}

void pmaf_k_launch_obs_slack_audit(const DevView &D, const ObsSlackArgs &A, const FTrackArgs *F, hipStream_t s) {
  const dim3 grid((unsigned)D.N, (unsigned)D.P), block(64 * PMAF_SELECT_WAVES);
  if (F) hipLaunchKernelGGL(k_obs_slack_audit<true>, grid, block, 0, s, D, A, *F);
  else hipLaunchKernelGGL(k_obs_slack_audit<false>, grid, block, 0, s, D, A, FTrackArgs{});
}
