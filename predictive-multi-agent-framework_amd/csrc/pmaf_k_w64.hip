// pmaf_k_w64.hip -- k_rollout_w64<TILES, MATH>: the wave-per-agent rollout kernel (latency shape: C1, C2, C3) and its
// launcher. Compiled once per arithmetic policy (-DPMAF_W64_MATH=0|1|2|3, csrc/build.sh; 3 with -ffp-contract=fast) so the policies build in
// parallel; each object defines pmaf_k_launch_w64_m<policy>, pmaf_k_launch_w64 (pmaf_k_misc.hip) dispatches.
// The step itself (rollout_w64_body) and its dispatch live in pmaf_rollout_w64_body.hpp, which pmaf_k_track.hip and
// pmaf_k_ftrack.hip include as well.
#include "pmaf_rollout_w64_body.hpp"

template <int TILES, int MATH, bool DPPSUM, bool PLAIN>
__global__ __launch_bounds__(64) void k_rollout_w64(DevView D, CostParams CP) {
  rollout_w64_dispatch<TILES, MATH, DPPSUM, PLAIN, false>(D, CP);
}
// the one-slot kernel (DPP sum, PLAIN step) with the priority-slicing loop: launches with two waves on a SIMD (SLICE in
// the header). A kernel of its own so that k_rollout_w64's names -- what the rocprofv3 summaries and profiles/traffic.json are keyed by -- stay.
template <int MATH>
__global__ __launch_bounds__(64) void k_rollout_w64_sliced(DevView D, CostParams CP) {
  rollout_w64_dispatch<1, MATH, true, true, true>(D, CP);
}

#ifndef PMAF_W64_MATH
#error "compile with -DPMAF_W64_MATH=0|1|2|3"
#endif
#define PMAF_CAT2(a, b) a##b
#define PMAF_CAT(a, b) PMAF_CAT2(a, b)
// PMAF_W64_PART (csrc/build.sh, default policy only): the translation unit holds the one-slot kernels (1) or the
// multi-slot kernels (2) alone -- the two are compiled with different pre-RA scheduling directions (measured per
// kernel family: build.sh); undefined = all of them in one unit.
#if defined(PMAF_W64_PART) && PMAF_W64_PART == 1
#define PMAF_W64_LAUNCH PMAF_CAT(PMAF_CAT(pmaf_k_launch_w64_m, PMAF_W64_MATH), _t1)
#elif defined(PMAF_W64_PART) && PMAF_W64_PART == 2
#define PMAF_W64_LAUNCH PMAF_CAT(PMAF_CAT(pmaf_k_launch_w64_m, PMAF_W64_MATH), _tn)
#else
#define PMAF_W64_LAUNCH PMAF_CAT(pmaf_k_launch_w64_m, PMAF_W64_MATH)
#endif
bool PMAF_W64_LAUNCH(const DevView &D, const CostParams &cp, int tiles, bool dppsum,
                     bool plain, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, bool slice) {
  const dim3 g64((unsigned)D.N, (unsigned)D.P), block(64);
#define PMAF_L(K) hipExtLaunchKernelGGL(K, g64, block, (unsigned)lds, s, e0, e1, 0, D, cp)
  // one slot per lane: both ordered-sum variants (the host picks); two / four slots: DPP only
#define PMAF_LP(T, S) do { if (plain) PMAF_L((k_rollout_w64<T, PMAF_W64_MATH, S, true>)); \
                           else PMAF_L((k_rollout_w64<T, PMAF_W64_MATH, S, false>)); } while (0)
#if !defined(PMAF_W64_PART) || PMAF_W64_PART == 1
#if PMAF_W64_MATH >= 2
  // two waves per SIMD: the priority-slicing loop (one-slot, DPP sum, PLAIN -- what many-agent populations run)
  if (slice && tiles <= 1 && dppsum && plain) { PMAF_L((k_rollout_w64_sliced<PMAF_W64_MATH>)); return true; }
#endif
  if (tiles <= 1 && !dppsum) { PMAF_LP(1, false); return true; }
  if (tiles <= 1) { PMAF_LP(1, true); return true; }
#endif
#if !defined(PMAF_W64_PART) || PMAF_W64_PART == 2
  if (tiles == 2) { PMAF_LP(2, true); return true; }
  if (tiles > 2 && tiles <= 4) { PMAF_LP(4, true); return true; }
#endif
#undef PMAF_LP
#undef PMAF_L
  return false;
}
