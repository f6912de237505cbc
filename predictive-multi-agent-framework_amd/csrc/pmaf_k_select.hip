// pmaf_k_select.hip -- the kernels of pmaf_select_clear / pmaf_adopt_best (include/pmaf.h, "selection against the live
// list") and their launchers. A translation unit of its own, object select.o: the code objects of the other units stay
// byte for byte what they were (NOTES.md 1: code placement alone moves the rollout loop).
//
// The audit's contract and shape are written down once, in pmaf_select_audit.hpp.
//
// k_select_stage   the caller's list out of mapped pinned host memory into device scratch, once: the audit's N * P blocks
//                  would each read it over PCIe otherwise (uncached: 7 * n_obs round trips per wave).
// k_select_audit   select_audit_body<false, false> (pmaf_select_audit.hpp): no track code, one pass per obstacle tile.
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
// Three launches in stream order; no last-block-done counter. One launcher per kernel: the host (pmaf_host_audit.cpp)
// puts stage, an audit -- this unit's or one of pmaf_k_auditft.hip's -- and the pick in a row.
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_adopt.hpp"
#include "pmaf_select_audit.hpp"

using namespace pmaf;

__global__ __launch_bounds__(256) void k_select_stage(int total, const double *src, double *dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) dst[i] = __builtin_nontemporal_load(src + i);
}

__global__ __launch_bounds__(64 * PMAF_SELECT_WAVES) void k_select_audit(DevView D, SelectArgs A) {
  select_audit_body<false, false>(D, A, FTrackArgs{}, 0ull);
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

void pmaf_k_launch_select_stage(const DevView &D, const SelectArgs &A, hipStream_t s) {
  const int total = D.P * 7 * D.n_obs;
  hipLaunchKernelGGL(k_select_stage, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, A.obs_src, A.obs);
}

void pmaf_k_launch_select_audit(const DevView &D, const SelectArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_select_audit, dim3((unsigned)D.N, (unsigned)D.P), dim3(64 * PMAF_SELECT_WAVES), 0, s, D, A);
}

void pmaf_k_launch_select_pick(const DevView &D, const SelectArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_select_pick, dim3((unsigned)D.P), dim3(64), 0, s, D, A);
}

void pmaf_k_launch_adopt_best(const DevView &D, const AdoptArgs &A, hipStream_t s) {
  hipLaunchKernelGGL(k_adopt_best, dim3((unsigned)D.P), dim3(64), 0, s, D, A);
}
