// pmaf_track.hpp -- the repulsive track (include/pmaf.h "repulsive track"): the structs and the launch interface between
// pmaf_host.cpp and pmaf_k_track.hip. A header of its own so that no other kernel unit's inputs change with it.
#pragma once
#include "pmaf_types.hpp"

// What k_rollout_w64_track takes beside DevView / CostParams (DevView itself does not grow: every kernel takes it by
// value). Population p's track is track + p * max_len * 3, its length len[p] (0: none -- the straight line as ever).
struct TrackArgs {
  const double *track;   // [P][max_len][3]
  const int32_t *len;    // [P]
  int max_len;           // >= 1
};

// k_track_from_best: population p with src_pop[p] = q >= 0 gets the selected path of q -- agent best_idx[q] as it lies in
// `paths` -- from point `shift` on: len = max(n_points - shift, 1) (a path of no more than `shift` points: its last
// point alone), 0 while q has no selection (has_best[q] == 0). max_len >= DevView::cap.
struct CoupleArgs {
  const int32_t *src_pop;   // [P], < 0: not coupled (the block leaves the population's track alone)
  const double *paths;      // [P][N][cap][3]: the buffer the selection scored
  double *track;            // [P][max_len][3]
  int32_t *len;             // [P]
  int max_len, shift;
};

// k_rollout_w64_track<DPPSUM, PLAIN> on grid (N, P): the one-slot wave-per-agent kernel of the default arithmetic policy
// (<= 60 field obstacles). e0 / e1 as for pmaf_k_launch_w64.
bool pmaf_k_launch_w64_track(const DevView &D, const CostParams &cp, const TrackArgs &T, bool dppsum, bool plain, size_t lds,
                             hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// k_track_from_best on grid P
void pmaf_k_launch_track_from_best(const DevView &D, const CoupleArgs &A, hipStream_t s);
