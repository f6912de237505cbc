// pmaf_k_select.hip -- the kernels of pmaf_select_clear / pmaf_adopt_best (include/pmaf.h, "selection against the live
// list") and their launchers. A translation unit of its own, object select.o: the code objects of the other units stay
// byte for byte what they were (NOTES.md 1: code placement alone moves the rollout loop).
//
// Semantics (the host-side contract is in include/pmaf.h). For agent (p, a) with n = n_points[p][a] the audit window is
// the first w = min(n, horizon) points of the current path; inside it everything is pmaf_evaluate_paths' contract:
//   o_j^0 = the caller's position, o_j^{k+1} = o_j^k + v_j * dt   (one multiply, one add per component, each rounded)
//   c(k, j) = norm(x_k - o_j^k) - (rad + r_j)                     (the build's dot association; no floor, no cap)
//   c_a  = min over k < w and j by a strict `<` from +inf (a NaN pair never wins), +inf for w = 0
//   fv_a = the smallest k < w with c(k, j) < margin for some j, else w;    clear_a <=> fv_a == w
// and the pick over a population's agents is the rule of pmaf.h (rule 0 keep / 1 cheapest clear / 2 fallback).
//
// k_select_stage   the caller's list out of mapped pinned host memory into device scratch, once: the audit's N * P blocks
//                  would each read it over PCIe otherwise (uncached: 7 * n_obs round trips per wave).
// k_select_audit   one block of four waves per (agent, population); lane = obstacle j of a tile of 64; the four waves
//                  take the four quarters [q * ceil(w / 4), (q + 1) * ceil(w / 4)) of the window.
//                   - no track buffer: the lane keeps its obstacle's position in three registers and advances it by the
//                     pre-rounded s = v * dt, one add per component and step. v * dt is the same rounded product in every
//                     step of k_audit_track's chain (-ffp-contract=off: the multiply and the add are never fused), so
//                     hoisting it changes no bit; and the chain o^{k+1} = o^k + s is walked from o^0 in the same order,
//                     so o^k has k_audit_track's bits for every k. A wave that starts at step k0 first walks the k0 adds
//                     of the chain alone (3 adds per step against ~50 operations of an audited step).
//                   - the path point is a wave-uniform load; horizon bounds the loop (the caller's lever at tick rate).
//                   - reductions are minima of doubles (no NaN ever enters one) and of integers: exact, associative and
//                     commutative, so neither the split over waves nor the lane butterflies change a bit. No atomics.
// k_select_pick    one wave per population strides over the agents as k_manager's argmin does: the cheapest clear agent
//                  (strict `<` from +inf per lane over ascending index, then group_argmin: ties to the smallest index,
//                  +inf and NaN never win), the number of clear agents (integer sum), and the fallback's maximum under
//                  the total order (fv, c, -index) -- c is never NaN, so the order is total and the butterfly finds what
//                  the ascending strict scan finds. Then the rule, the result record into mapped pinned host memory
//                  behind a sequence number (as k_manager's mailbox), and -- when asked -- the adopt stores.
// k_adopt_best     the adopt stores alone, one wave per population: k_manager's `take` block
//                  (best_agent_ = ee_agents_[i]->makeCopy(), B/src/cf_manager.cpp:346; adopt_agent, pmaf_adopt.hpp).
// The joint selection (pmaf_k_pairclear.hip) launches k_select_stage and k_select_audit as they are and hands the audit
// SelectArgs::n_audit = n_obs - 1 when it leaves the trailing obstacle to the cross audit; pmaf_select_clear passes n_obs.
// Three launches in stream order; no last-block-done counter.
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_adopt.hpp"

using namespace pmaf;

#define PMAF_SELECT_WAVES 4

__global__ __launch_bounds__(256) void k_select_stage(int total, const double *src, double *dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) dst[i] = __builtin_nontemporal_load(src + i);
}

__global__ __launch_bounds__(64 * PMAF_SELECT_WAVES) void k_select_audit(DevView D, SelectArgs A) {
  __shared__ double s_c[PMAF_SELECT_WAVES];
  __shared__ int s_v[PMAF_SELECT_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pop = blockIdx.y, a = blockIdx.x;
  const int n_obs = D.n_obs;       // the lists' stride
  const int n_audit = A.n_audit;   // the audited obstacles: n_obs, or n_obs - 1 (the joint selection skips the trailing one)
  PMAF_BOUND(n_audit >= 0 && n_audit <= n_obs);
  const size_t pa = (size_t)pop * D.N + a;
  int n = D.n_points[pa];
  PMAF_BOUND(n >= 0 && n <= D.cap);
  n = n < D.cap ? n : D.cap;
  PMAF_BOUND(A.horizon >= 1 && A.horizon <= D.cap);
  const int w = n < A.horizon ? n : A.horizon;
  // this wave's quarter of the window (block-uniform w, wave-uniform bounds)
  const int chunk = (w + PMAF_SELECT_WAVES - 1) / PMAF_SELECT_WAVES;
  const int k0 = wave * chunk < w ? wave * chunk : w;
  const int k1 = k0 + chunk < w ? k0 + chunk : w;
  const double *path = D.paths + pa * (size_t)D.cap * 3;
  const double *o = A.obs + (size_t)pop * 7 * n_obs;
  const double dt = D.C.dt;
  const double inf = __builtin_huge_val();

  double best = inf;
  int viol = 0x7fffffff;
  if (k0 < k1) {
    for (int j0 = 0; j0 < n_audit; j0 += 64) {   // one pass over the quarter per obstacle tile
      const int j = j0 + lane;
      const bool jv = j < n_audit;
      const int jc = jv ? j : 0;
      V3 q = mk(o[jc], o[n_obs + jc], o[2 * (size_t)n_obs + jc]);
      // predictObstacles' v * dt, rounded once: the same double in every step of the chain
      const V3 s = mk(o[3 * (size_t)n_obs + jc] * dt, o[4 * (size_t)n_obs + jc] * dt, o[5 * (size_t)n_obs + jc] * dt);
      const double rr = D.C.rad + o[6 * (size_t)n_obs + jc];
      for (int k = 0; k < k0; k++) {   // the chain up to this wave's first step
        q.x = q.x + s.x;
        q.y = q.y + s.y;
        q.z = q.z + s.z;
      }
      for (int k = k0; k < k1; k++) {
        const V3 x = mk(path[k * 3], path[k * 3 + 1], path[k * 3 + 2]);
        const double c = norm(x - q) - rr;
        if (jv) {
          if (c < best) best = c;
          if (c < A.margin && k < viol) viol = k;
        }
        q.x = q.x + s.x;
        q.y = q.y + s.y;
        q.z = q.z + s.z;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oc = __shfl_xor(best, off);
    const int ov = __shfl_xor(viol, off);
    best = (oc < best) ? oc : best;
    viol = (ov < viol) ? ov : viol;
  }
  if (lane == 0) { s_c[wave] = best; s_v[wave] = viol; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 1; q < PMAF_SELECT_WAVES; q++) {
      const double oc = s_c[q];
      const int ov = s_v[q];
      best = (oc < best) ? oc : best;
      viol = (ov < viol) ? ov : viol;
    }
    A.clr[pa] = best;
    A.fv[pa] = (viol == 0x7fffffff) ? w : viol;
  }
}

__global__ __launch_bounds__(64) void k_select_pick(DevView D, SelectArgs A) {
  const int lane = threadIdx.x;
  const int pop = blockIdx.x;
  const int N = D.N;
  const double inf = __builtin_huge_val();
  const int none = 0x7fffffff;

  double lmin = inf;       // cheapest clear agent of this lane
  int lidx = none;
  int n_clear = 0;
  int f_fv = -1, f_idx = none;   // fallback: greatest fv, then greatest c, then smallest index
  double f_c = -inf;
  for (int a = lane; a < N; a += 64) {
    const size_t pa = (size_t)pop * N + a;
    int n = D.n_points[pa];
    n = n < D.cap ? n : D.cap;
    const int w = n < A.horizon ? n : A.horizon;
    const int fv = A.fv[pa];
    const double c = A.clr[pa];
    const double cost = D.costs[pa];
    const bool clear = fv == w;
    n_clear += clear ? 1 : 0;
    if (clear && cost < lmin) { lmin = cost; lidx = a; }
    if (fv > f_fv || (fv == f_fv && c > f_c)) { f_fv = fv; f_c = c; f_idx = a; }
  }
  group_argmin<64>(lmin, lidx);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_clear += __shfl_xor(n_clear, off);
    const int ofv = __shfl_xor(f_fv, off), oi = __shfl_xor(f_idx, off);
    const double oc = __shfl_xor(f_c, off);
    const bool take = ofv > f_fv || (ofv == f_fv && (oc > f_c || (oc == f_c && oi < f_idx)));
    f_fv = take ? ofv : f_fv;
    f_c = take ? oc : f_c;
    f_idx = take ? oi : f_idx;
  }
  int pick, rule;
  if (lidx != none) {
    pick = lidx;
    rule = 1;
    const int q = A.prev ? A.prev[pop] : -1;
    PMAF_BOUND(q >= -1 && q < N);
    if (q >= 0 && q < N) {
      const size_t pq = (size_t)pop * N + q;
      int nq = D.n_points[pq];
      nq = nq < D.cap ? nq : D.cap;
      const int wq = nq < A.horizon ? nq : A.horizon;
      const double cq = D.costs[pq];
      // evaluateAgents' hysteresis (B/src/cf_manager.cpp:344-350) on the clear set; a NaN cost of q fails the `>=`
      if (A.fv[pq] == wq && lmin >= 0.9 * cq) { pick = q; rule = 0; }
    }
  } else {
    pick = f_idx;   // N >= 1 and every agent beats the initial fv = -1: f_idx is in [0, N)
    rule = 2;
  }
  PMAF_BOUND(pick >= 0 && pick < N);
  const size_t pp = (size_t)pop * N + pick;
  if (A.adopt) adopt_agent(D, pop, pick, lane);
  double *r = A.result + (size_t)pop * PMAF_SELECT_REC;
  if (lane == 0) {
    r[0] = (double)pick;
    r[1] = (double)rule;
    r[2] = (double)n_clear;
    r[3] = (double)A.fv[pp];
    r[4] = D.costs[pp];
    r[5] = A.clr[pp];
  }
  __threadfence_system();   // the record (and the adopt stores) before the sequence number
  if (lane == 0) *reinterpret_cast<volatile double *>(r + 7) = A.seq;
}

__global__ __launch_bounds__(64) void k_adopt_best(DevView D, AdoptArgs A) {
  const int pop = blockIdx.x;
  const int i = A.idx ? A.idx[pop] : A.idx_val[pop];
  PMAF_BOUND(i >= -1 && i < D.N);
  if (i < 0 || i >= D.N) return;   // -1: this population keeps its best agent
  adopt_agent(D, pop, i, threadIdx.x);
}

void pmaf_k_launch_select_audit(const DevView &D, const SelectArgs &A, hipStream_t s) {
  const int total = D.P * 7 * D.n_obs;
  hipLaunchKernelGGL(k_select_stage, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, A.obs_src, A.obs);
  hipLaunchKernelGGL(k_select_audit, dim3((unsigned)D.N, (unsigned)D.P), dim3(64 * PMAF_SELECT_WAVES), 0, s, D, A);
}

void pmaf_k_launch_select_clear(const DevView &D, const SelectArgs &A, hipStream_t s) {
  pmaf_k_launch_select_audit(D, A, s);
  hipLaunchKernelGGL(k_select_pick, dim3((unsigned)D.P), dim3(64), 0, s, D, A);
}

// the first and the last of the three alone (pmaf_auditft.hpp): the tracked selection puts its own audit between them
void pmaf_k_launch_select_stage(const DevView &D, const SelectArgs &A, hipStream_t s) {
  const int total = D.P * 7 * D.n_obs;
  hipLaunchKernelGGL(k_select_stage, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, A.obs_src, A.obs);
}

void pmaf_k_launch_select_pick(const DevView &D, const SelectArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_select_pick, dim3((unsigned)D.P), dim3(64), 0, s, D, A);
}

void pmaf_k_launch_adopt_best(const DevView &D, const AdoptArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_adopt_best, dim3((unsigned)D.P), dim3(64), 0, s, D, A);
}
