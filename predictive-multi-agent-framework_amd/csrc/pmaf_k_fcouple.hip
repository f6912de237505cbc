// pmaf_k_fcouple.hip -- the obstacle tracks' device-side source (include/pmaf.h "obstacle tracks",
// pmaf_couple_obstacle_tracks): field obstacles that ride on another population's selected path. Two kernels for the
// composition's two moments, and their launchers. A translation unit of its own, object fcouple.o: the code objects of
// the other units stay byte for byte what they were (NOTES.md 1: code placement alone moves the rollout loop).
//
// k_fcouple_take     at the capture moment (where k_track_from_best runs: pmaf_reset_agents of the five-call tick,
//                    otherwise the rollout launch -- before a reset or the rollout rewrites the paths): one block per
//                    population; a SOURCE population q copies the path of agent best_idx[q] from point min(shift, n - 1)
//                    on into the staging buffer [P][cap][3] and stores n_c = max(n - shift, 1), or 0 while q has no
//                    selection. k_track_from_best's rule, clamps included.
// k_fcouple_compose  in front of the rollout, when obs_start is what the rollout will read: grid (chunks of
//                    PMAF_FCOUPLE_CHUNK points, population), one wave per block, lane = column of the layout
//                    [P][max_len][6][64] (pmaf_ftrack.hpp) -- each of a point's six rows is one contiguous 512-byte
//                    store. No dependent loads from point to point:
//                     - an attached lane (src >= 0 and its source has a selection) reads y_k and y_{k+1} of the staged
//                       path -- lanes attached to the same source read one address -- and forms
//                       x_k = RN(anchor + RN(scale y_k)), u_k = RN(RN(x_{k+1} - x_k) / dt) with the correctly rounded
//                       division of the default arithmetic policy (Mth<MATH_XACT>::div; the compiler's expansion is
//                       1 ulp low for three divisor mantissas, pmaf_device.hpp); from point n_c - 1 on the position is
//                       held and the velocity is +0.0. x_{k+1} is carried into the next point.
//                     - an unattached lane < M walks the list's chain q_{k+1} = RN(q_k + RN(v dt)) from obs_start: the
//                       k0 prefix adds up to its chunk, then the chunk (the way k_ft_select_audit carries the trailing
//                       obstacle's chain). Its velocity is the list's, constant.
//                     - lanes >= M store zeros.
//                    The block of chunk 0 stores len = cap (0 when no attached column's source has a selection: the
//                    population then rolls out untracked) and first = 0. A population without an attached column
//                    returns before any store: its part of the buffer -- an uploaded set of tracks -- is never touched.
// No atomics, no LDS, no scratch (tests/test_field_couple.py reads the resource record). Compiled with the plain kernel
// flags: -ffp-contract=off keeps the multiply and the add of x_k two roundings.
// (The names contain none of k_track_from_best, k_audit_track, k_rollout_w64_ftrack, k_select_audit and are contained in
// none: the other modules' tests find those lines of the resource record by substring and expect exactly one.)
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_fcouple.hpp"

using namespace pmaf;

__global__ __launch_bounds__(64) void k_fcouple_take(DevView D, FCoupleArgs A) {
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  if (A.is_src[q] == 0) return;
  if (D.has_best[q] == 0) {
    if (lane == 0) A.sel_n[q] = 0;
    return;
  }
  int b = D.best_idx[q];
  b = (b < 0) ? 0 : ((b >= D.N) ? D.N - 1 : b);
  const size_t qa = (size_t)q * D.N + b;
  int n = D.n_points[qa];
  n = (n < 1) ? 1 : ((n > D.cap) ? D.cap : n);
  const int first = (A.shift < n - 1) ? A.shift : (n - 1);
  const int n_c = n - first;   // == max(n - shift, 1), <= cap
  const double *src = A.paths + (qa * (size_t)D.cap + (size_t)first) * 3;
  double *dst = A.sel_pts + (size_t)q * D.cap * 3;
  for (int i = lane; i < 3 * n_c; i += 64) dst[i] = src[i];
  if (lane == 0) A.sel_n[q] = n_c;
}

__global__ __launch_bounds__(64) void k_fcouple_compose(DevView D, FCoupleArgs A) {
  using M = Mth<MATH_XACT>;
  const int lane = threadIdx.x;
  const int pop = blockIdx.y;
  const int n_obs = D.n_obs, nf = n_obs - 1;   // nf: the field obstacles (M of the contract)
  const int cap = D.cap;
  PMAF_BOUND(nf >= 0 && nf <= PMAF_FTRACK_LANES && A.max_len >= cap);
  int q = A.src[pop * PMAF_FTRACK_LANES + lane];
  q = (lane < nf && q >= 0 && q < D.P) ? q : -1;
  if (!wave_any(q >= 0)) return;   // not a coupled population: nothing of it is touched
  int n_c = (q >= 0) ? A.sel_n[q] : 0;
  n_c = (n_c < 0) ? 0 : ((n_c > cap) ? cap : n_c);
  const bool att = n_c > 0;
  const bool tracked = wave_any(att);   // block-uniform
  const int k0 = blockIdx.x * PMAF_FCOUPLE_CHUNK;
  if (k0 == 0 && lane == 0) {
    A.len[pop] = tracked ? cap : 0;
    A.first[pop] = 0;
  }
  if (!tracked || k0 >= cap) return;
  const int k1 = (k0 + PMAF_FCOUPLE_CHUNK < cap) ? k0 + PMAF_FCOUPLE_CHUNK : cap;
  const double dt = D.C.dt;
  const bool field = lane < nf;
  const int jc = field ? lane : 0;   // (the list's loads only)
  const double *o = D.obs_start + (size_t)pop * 7 * n_obs;
  V3 ql = mk(o[jc], o[n_obs + jc], o[2 * (size_t)n_obs + jc]);
  const V3 v = mk(o[3 * (size_t)n_obs + jc], o[4 * (size_t)n_obs + jc], o[5 * (size_t)n_obs + jc]);
  // predictObstacles' v * dt, rounded once: the same double in every step of the chain
  const V3 s = mk(v.x * dt, v.y * dt, v.z * dt);
  for (int k = 0; k < k0; k++) {   // the chain up to this block's first point
    ql.x = ql.x + s.x;
    ql.y = ql.y + s.y;
    ql.z = ql.z + s.z;
  }
  const double sc = A.scale[pop * PMAF_FTRACK_LANES + lane];
  const double *an = A.anchor + (size_t)pop * 3 * PMAF_FTRACK_LANES + lane;
  const V3 anc = mk(an[0], an[PMAF_FTRACK_LANES], an[2 * PMAF_FTRACK_LANES]);
  const double *y = A.sel_pts + (size_t)(att ? q : 0) * cap * 3;
  const int last = att ? n_c - 1 : 0;
  // x_i = RN(anchor + RN(scale * y_i)) of the held index min(i, n_c - 1); an unattached lane reads point 0 of
  // population 0's staging (inside the buffer) and drops the value
  auto point = [&](int i) {
    const int ii = (i < last) ? i : last;
    const double m0 = sc * y[3 * ii], m1 = sc * y[3 * ii + 1], m2 = sc * y[3 * ii + 2];
    return mk(anc.x + m0, anc.y + m1, anc.z + m2);
  };
  V3 xn = point(k0);
  double *dst = A.pts + ((size_t)pop * A.max_len + k0) * PMAF_FTRACK_POINT + lane;
  for (int k = k0; k < k1; k++) {
    const V3 x = xn;
    xn = point(k + 1);
    V3 u = mk(0.0, 0.0, 0.0);
    if (k < last) u = mk(M::div(xn.x - x.x, dt), M::div(xn.y - x.y, dt), M::div(xn.z - x.z, dt));
    const V3 p = att ? x : ql;
    const V3 w = att ? u : v;
    dst[0] = field ? p.x : 0.0;
    dst[PMAF_FTRACK_LANES] = field ? p.y : 0.0;
    dst[2 * PMAF_FTRACK_LANES] = field ? p.z : 0.0;
    dst[3 * PMAF_FTRACK_LANES] = field ? w.x : 0.0;
    dst[4 * PMAF_FTRACK_LANES] = field ? w.y : 0.0;
    dst[5 * PMAF_FTRACK_LANES] = field ? w.z : 0.0;
    dst += PMAF_FTRACK_POINT;
    ql.x = ql.x + s.x;
    ql.y = ql.y + s.y;
    ql.z = ql.z + s.z;
  }
}

void pmaf_k_launch_fcouple_take(const DevView &D, const FCoupleArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_fcouple_take, dim3((unsigned)D.P), dim3(64), 0, s, D, A);
}

void pmaf_k_launch_fcouple_compose(const DevView &D, const FCoupleArgs &A, hipStream_t s) {
  const unsigned chunks = (unsigned)((D.cap + PMAF_FCOUPLE_CHUNK - 1) / PMAF_FCOUPLE_CHUNK);
  hipLaunchKernelGGL(k_fcouple_compose, dim3(chunks, (unsigned)D.P), dim3(64), 0, s, D, A);
}
