// pmaf_fcouple.hpp -- the obstacle tracks' device-side source (include/pmaf.h "obstacle tracks",
// pmaf_couple_obstacle_tracks): the struct and the launch interface between pmaf_host.cpp and pmaf_k_fcouple.hip. A header
// of its own so that no other kernel unit's inputs change with it.
#pragma once
#include "pmaf_types.hpp"
#include "pmaf_ftrack.hpp"

// Field obstacle i < M of population p with src[p][i] = q >= 0 rides on the selected path of population q: at point k its
// position is anchor + scale * y_k (one rounded multiply, one rounded add), y_k = point k of that path from point `shift`
// on, held at the end; its velocity the forward difference over dt, +0.0 from the last point on. The per-column inputs are
// padded to the wave (PMAF_FTRACK_LANES columns; src = -1, scale = anchor = 0 behind M) so that lane = column reads them
// without a bound of its own.
struct FCoupleArgs {
  const int32_t *src;       // [P][64], < 0: the column keeps the straight line of the rollout-start list
  const double *scale;      // [P][64]
  const double *anchor;     // [P][3][64]
  const int32_t *is_src;    // [P], != 0: some column of this handle rides on this population's selected path
  const double *paths;      // [P][N][cap][3]: the buffer the selection scored (k_fcouple_take only)
  double *sel_pts;          // [P][cap][3] staging: the selected path of a source population from point `shift` on ...
  int32_t *sel_n;           // [P] ... and its point count n_c = max(n_points - shift, 1); 0: no selection yet
  double *pts;              // [P][max_len][6][64]  (pmaf_ftrack.hpp; k_fcouple_compose only, as the two below)
  int32_t *len, *first;     // [P]
  int max_len, shift;       // max_len >= DevView::cap
};

// points of the tracks one block of k_fcouple_compose writes
#define PMAF_FCOUPLE_CHUNK 8

// k_fcouple_take on grid P: a source population's selected path -- agent best_idx[q] as it lies in `paths` -- into the
// staging buffer; populations that are no source are left alone.
void pmaf_k_launch_fcouple_take(const DevView &D, const FCoupleArgs &A, hipStream_t s);
// k_fcouple_compose on grid (ceil(cap / PMAF_FCOUPLE_CHUNK), P): the coupled populations' points of the tracks, their
// len (cap, or 0 while no attached column's source has a selection) and first (0) from the staging buffer and
// DevView::obs_start; a population without an attached column is not touched.
void pmaf_k_launch_fcouple_compose(const DevView &D, const FCoupleArgs &A, hipStream_t s);
