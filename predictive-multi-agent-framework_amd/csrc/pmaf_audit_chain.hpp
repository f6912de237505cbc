// pmaf_audit_chain.hpp -- the obstacle chain of the path audit's track buffer as a device function, for the untracked
// columns of k_audit_track_ft (pmaf_k_auditft.hip). No kernel: a unit that includes it gains no code object entry.
// k_audit_track (pmaf_path_audit.hpp) walks the same chain in its own text: called from there, this function moved the
// kernel's address arithmetic, and with it k_misc.o, which also holds k_manager (NOTES.md 1, experiments not kept).
#pragma once
#include "pmaf_types.hpp"
#include "pmaf_device.hpp"

namespace pmaf {

// obstacle j of the list o [7][n_obs] at steps 0 .. cap-1 into its column t of the rows [cap][3][n_obs]:
// o^0 = the caller's position, o^{k+1} = o^k + v * dt (one multiply, one add per component, each rounded)
__device__ __forceinline__ void audit_track_chain(const double *o, int n_obs, int j, int cap, double dt, double *t) {
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

}  // namespace pmaf
