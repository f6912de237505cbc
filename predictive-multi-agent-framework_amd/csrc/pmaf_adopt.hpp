// pmaf_adopt.hpp -- the adopt stores, shared by the units that make a pick the population's best agent:
// pmaf_k_select.hip (k_select_pick, k_adopt_best) and pmaf_k_pairclear.hip (k_pairclear_final). No kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"

// k_manager's `take` block for agent i of population pop
__device__ __forceinline__ void adopt_agent(const DevView &D, int pop, int i, int lane) {
  const int n_obs = D.n_obs;
  const double *src = D.rnd + ((size_t)pop * D.N + i) * 3 * n_obs;
  double *dst = D.best_rnd + (size_t)pop * 3 * n_obs;
  for (int e = lane; e < 3 * n_obs; e += 64) dst[e] = src[e];
  if (lane == 0) {
    D.has_best[pop] = 1;
    D.best_id[pop] = i + 1;
    D.best_type[pop] = D.types[i];
    D.best_idx[pop] = i;
  }
}
