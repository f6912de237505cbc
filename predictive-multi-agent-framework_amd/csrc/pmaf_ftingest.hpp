// pmaf_ftingest.hpp -- the obstacle tracks' device-memory source (include/pmaf.h "obstacle tracks",
// pmaf_set_obstacle_tracks_device): the struct and the launch interface between pmaf_host.cpp and pmaf_k_ftingest.hip. A
// header of its own so that no other kernel unit's inputs change with it.
#pragma once
#include "pmaf_types.hpp"
#include "pmaf_ftrack.hpp"

// The caller's tracks lie in memory the device reads: [P][src_max][M][comps] elements of `dtype` (PMAF_TRACK_F64 /
// PMAF_TRACK_F32 of include/pmaf.h), comps 6 (position and velocity, verbatim) or 3 (positions; the velocity of point
// k < len - 1 is RN(RN(x_{k+1} - x_k) / dt), +0.0 at point len - 1). Of population p exactly the leading
// len[p] * M * comps elements of its slab are read. len[p] < 0: the population is not touched (a coupled population:
// its points are k_fcouple_compose's).
struct FtIngestArgs {
  const void *src;
  const int32_t *len;            // [P], device memory: the caller's lengths, -1 for a population that is left alone
  double *pts;                   // [P][stride][6][64]  (pmaf_ftrack.hpp)
  unsigned long long *verdict;   // one word: the smallest key of an offending value, PMAF_FTINGEST_CLEAN: none
  int src_max, stride;           // 1 <= src_max <= stride
  int M;                         // field obstacles, <= PMAF_FTRACK_LANES
  double dt;                     // DevView::C.dt
};

// The verdict's key: the flat index of a value in the INGESTED order [P][src_max][M][6] -- for comps == 6 the source
// order; for comps == 3 a derived velocity (components 3 .. 5) counts at its point, behind its obstacle's positions. A
// derived velocity is judged only where both positions it is taken from pass themselves: a position that is out of
// range is named itself, not through the difference it spoils.
#define PMAF_FTINGEST_CLEAN (~0ull)

// points of the tracks one block walks (one wave, lane = column: for comps == 3 point k + 1 is loaded once and carried)
#define PMAF_FTINGEST_CHUNK 8

// k_ftingest_check<T, C> on grid (ceil(src_max / PMAF_FTINGEST_CHUNK), P): the range rule of check_range
// (pmaf_host_impl.hpp) on every ingested value after widening; an offender's key goes into *verdict by atomic minimum
// (deterministic: the first in the order above, whichever lane gets there first). The caller sets *verdict to
// PMAF_FTINGEST_CLEAN in front. Writes nothing else.
// k_ftingest_store<T, C> on the same grid, behind it in stream order: returns at once unless *verdict is
// PMAF_FTINGEST_CLEAN (a refused set of tracks leaves the buffer as it was); otherwise the transposition into pts -- each
// of a point's six rows one contiguous 512-byte store, columns >= M zero -- of the points k < len[p], and one zero
// point for a population of length 0 (the point the rollout's loads may touch).
// comps, dtype: validated by the caller (3 | 6, PMAF_TRACK_F64 | PMAF_TRACK_F32).
void pmaf_k_launch_ftingest(const FtIngestArgs &A, int P, int comps, int dtype, hipStream_t s);
