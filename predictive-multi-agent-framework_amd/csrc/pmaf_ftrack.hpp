// pmaf_ftrack.hpp -- the obstacle tracks (include/pmaf.h "obstacle tracks"): the struct and the launch interface between
// pmaf_host.cpp and pmaf_k_ftrack.hip. A header of its own so that no other kernel unit's inputs change with it.
#pragma once
#include "pmaf_types.hpp"
#include "pmaf_track.hpp"

// Device layout of the tracks: [P][max_len][6][PMAF_FTRACK_LANES] doubles -- per point the six components (position x y z,
// velocity x y z), each a row of one double per lane of the wave: lane i < M reads obstacle i's, at a fixed offset from
// its own pointer, and a wave's load of one component is one contiguous row. Columns >= M are zero and never used.
#define PMAF_FTRACK_LANES 64
#define PMAF_FTRACK_POINT (6 * PMAF_FTRACK_LANES)   // doubles per point

// What k_rollout_w64_ftrack takes beside DevView / CostParams / TrackArgs (DevView does not grow). Population p's tracks
// are pts + p * max_len * PMAF_FTRACK_POINT, len[p] points (0: none -- the straight lines as ever), read from point
// first[p] on: step k sees point min(first[p] + k, len[p] - 1).
struct FTrackArgs {
  const double *pts;      // [P][max_len][6][64]
  const int32_t *len;     // [P]
  const int32_t *first;   // [P], >= 0
  int max_len;            // >= 1: a population without tracks still has one (zero) point the loads may touch
};

// k_rollout_w64_ftrack<DPPSUM, PLAIN> on grid (N, P): the one-slot wave-per-agent kernel of the default arithmetic policy
// (<= 60 field obstacles) whose field obstacles follow F and whose trailing obstacle follows T (either may be empty:
// len 0 for every population, but both buffers exist). e0 / e1 as for pmaf_k_launch_w64.
bool pmaf_k_launch_w64_ftrack(const DevView &D, const CostParams &cp, const TrackArgs &T, const FTrackArgs &F, bool dppsum,
                              bool plain, size_t lds, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
