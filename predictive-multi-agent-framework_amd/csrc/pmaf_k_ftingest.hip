// pmaf_k_ftingest.hip -- the obstacle tracks' device-memory source (include/pmaf.h "obstacle tracks",
// pmaf_set_obstacle_tracks_device): tracks that a predictor on the same device has written are range-checked, widened,
// differenced and transposed where they lie, instead of travelling to the host and back. Two kernels, each in four
// instances (element type double | float, components 6 | 3), and their launcher. A translation unit of its own, object
// ftingest.o: the code objects of the other units stay byte for byte what they were (NOTES.md 1).
//
// Both kernels walk the same way (ft_walk): grid (chunks of PMAF_FTINGEST_CHUNK points, population), one wave per block,
// lane = column of the layout [P][stride][6][64] (pmaf_ftrack.hpp). Lane i < M reads obstacle i's C adjacent elements of
// a point with loads of the element's own alignment (a source that is 8-aligned but not 16-aligned is legal); the wave's
// loads of one point cover its contiguous source row of M * C elements. With C == 3 point k + 1 is loaded once and
// carried into the next point; only the block's first point is read by two blocks. Nothing behind len[p] * M * C
// elements of a population's slab is read.
//   velocity, C == 3   u_k = RN(RN(x_{k+1} - x_k) / dt) per component with the correctly rounded division of the default
//                      arithmetic policy (Mth<MATH_XACT>::div, as k_fcouple_compose), +0.0 at point len - 1
// k_ftingest_check   the range rule on every ingested value (finite; 0 or 2^-100 <= |x| <= 2^100, after widening, the
//                    derived velocities included): a lane that meets an offender takes the smallest key of its own
//                    (pmaf_ftingest.hpp) and folds it into the verdict word with one atomic minimum -- no lane on valid
//                    tracks. Stores nothing else.
// k_ftingest_store   behind it in stream order: returns unless the verdict is clean; otherwise each of a point's six
//                    rows is one contiguous 512-byte store, columns >= M zero; a population of length 0 gets one zero
//                    point, a population of length < 0 is not touched.
// No LDS, no scratch (tests/test_track_ingest.py reads the resource record). Compiled with the plain kernel flags:
// -ffp-contract=off keeps the difference and the division two roundings.
// (The names contain none of k_track_from_best, k_audit_track, k_rollout_w64_ftrack, k_select_audit, k_fcouple_ and are
// contained in none: the other modules' tests find those lines of the resource record by substring.)
#include <hip/hip_runtime.h>

#include "../../include/pmaf.h"
#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_ftingest.hpp"

using namespace pmaf;

// the widening is exact for every float, subnormals included
__device__ __forceinline__ double ft_widen(const double *p) { return *p; }
__device__ __forceinline__ double ft_widen(const float *p) { return (double)*p; }

// check_range's rule (pmaf_host_impl.hpp); a NaN fails every comparison
__device__ __forceinline__ bool ft_in_range(double x) {
  const double a = __builtin_fabs(x);
  return a == 0.0 || (a >= 0x1p-100 && a <= 0x1p100);
}

// The points k0 <= k < k1 of population `pop` as this lane's column holds them: f(k, have, v, xn) with v the six
// ingested values (zeros where have == false: a column >= M or a point >= L) and, for C == 3, xn the positions of point
// k + 1 the velocity was taken from (zeros at the last point).
template <typename T, int C, typename F>
__device__ __forceinline__ void ft_walk(const FtIngestArgs &A, int pop, int lane, int k0, int k1, int L, F &&f) {
  using M = Mth<MATH_XACT>;
  const bool col = lane < A.M;
  const size_t row = (size_t)A.M * C;
  const T *s = static_cast<const T *>(A.src) + ((size_t)pop * A.src_max + k0) * row + (size_t)(col ? lane : 0) * C;
  const double dt = A.dt;
  double xn[3] = {0.0, 0.0, 0.0};
  if (C == 3 && col && k0 < L) {
#pragma unroll
    for (int c = 0; c < 3; c++) xn[c] = ft_widen(s + c);
  }
  for (int k = k0; k < k1; k++) {
    const bool have = col && k < L;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (C == 6) {
      if (have) {
#pragma unroll
        for (int c = 0; c < 6; c++) v[c] = ft_widen(s + c);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = have ? xn[c] : 0.0;
      const bool nxt = col && k + 1 < L;
#pragma unroll
      for (int c = 0; c < 3; c++) xn[c] = nxt ? ft_widen(s + row + c) : 0.0;
      if (nxt) {
#pragma unroll
        for (int c = 0; c < 3; c++) v[3 + c] = M::div(xn[c] - v[c], dt);
      }
    }
    f(k, have, v, xn);
    s += row;
  }
}

template <typename T, int C>
__global__ __launch_bounds__(64) void k_ftingest_check(FtIngestArgs A) {
  const int lane = threadIdx.x;
  const int pop = blockIdx.y;
  PMAF_BOUND(A.M >= 0 && A.M <= PMAF_FTRACK_LANES && A.src_max >= 1);
  int L = A.len[pop];
  L = (L > A.src_max) ? A.src_max : L;
  const int k0 = blockIdx.x * PMAF_FTINGEST_CHUNK;
  if (k0 >= L) return;
  const int k1 = (k0 + PMAF_FTINGEST_CHUNK < L) ? k0 + PMAF_FTINGEST_CHUNK : L;
  unsigned long long key = PMAF_FTINGEST_CLEAN;
  ft_walk<T, C>(A, pop, lane, k0, k1, L, [&](int k, bool have, const double *v, const double *xn) {
    if (!have) return;
    const unsigned long long at = (((unsigned long long)pop * A.src_max + k) * A.M + lane) * 6;
#pragma unroll
    for (int c = 0; c < 6; c++) {
      // (at the last point v is +0.0 and passes whatever xn holds)
      const bool judged = (C == 6 || c < 3) ? true : ft_in_range(xn[c < 3 ? 0 : c - 3]);
      if (judged && !ft_in_range(v[c]) && key == PMAF_FTINGEST_CLEAN) key = at + c;
    }
  });
  if (key != PMAF_FTINGEST_CLEAN) atomicMin(A.verdict, key);
}

template <typename T, int C>
__global__ __launch_bounds__(64) void k_ftingest_store(FtIngestArgs A) {
  const int lane = threadIdx.x;
  const int pop = blockIdx.y;
  PMAF_BOUND(A.M >= 0 && A.M <= PMAF_FTRACK_LANES && A.src_max >= 1 && A.src_max <= A.stride);
  if (*A.verdict != PMAF_FTINGEST_CLEAN) return;
  int L = A.len[pop];
  if (L < 0) return;
  L = (L > A.src_max) ? A.src_max : L;
  const int n = (L > 1) ? L : 1;
  const int k0 = blockIdx.x * PMAF_FTINGEST_CHUNK;
  if (k0 >= n) return;
  const int k1 = (k0 + PMAF_FTINGEST_CHUNK < n) ? k0 + PMAF_FTINGEST_CHUNK : n;
  double *pts = A.pts + (size_t)pop * A.stride * PMAF_FTRACK_POINT + lane;
  ft_walk<T, C>(A, pop, lane, k0, k1, L, [&](int k, bool, const double *v, const double *) {
    double *dst = pts + (size_t)k * PMAF_FTRACK_POINT;
#pragma unroll
    for (int c = 0; c < 6; c++) dst[c * PMAF_FTRACK_LANES] = v[c];
  });
}

template <typename T, int C>
static void launch(const FtIngestArgs &A, int P, hipStream_t s) {
  const unsigned chunks = (unsigned)((A.src_max + PMAF_FTINGEST_CHUNK - 1) / PMAF_FTINGEST_CHUNK);
  hipLaunchKernelGGL((k_ftingest_check<T, C>), dim3(chunks, (unsigned)P), dim3(64), 0, s, A);
  hipLaunchKernelGGL((k_ftingest_store<T, C>), dim3(chunks, (unsigned)P), dim3(64), 0, s, A);
}

void pmaf_k_launch_ftingest(const FtIngestArgs &A, int P, int comps, int dtype, hipStream_t s) {
  if (dtype == PMAF_TRACK_F64) {
    if (comps == 6) launch<double, 6>(A, P, s);
    else launch<double, 3>(A, P, s);
  } else {
    if (comps == 6) launch<float, 6>(A, P, s);
    else launch<float, 3>(A, P, s);
  }
}
