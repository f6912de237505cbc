// pmaf_k_pairclear.hip -- the kernels of pmaf_select_pair_clear / pmaf_select_clear_tracks (include/pmaf.h, "joint
// selection: clear of the live list and of each other") and their launcher. A translation unit of its own, object
// pairclear.o: the code objects of the other units stay byte for byte what they were (NOTES.md 1: code placement alone
// moves the rollout loop). The audits themselves are not here: the call runs k_select_stage / k_select_audit
// (pmaf_k_select.hip) and k_cross_audit or k_cross_audit_slack as they are, and these kernels join their results.
//
// Semantics (the host-side contract is in include/pmaf.h). Side A is a population, side B a second population or the
// caller's tracks; w = min(n_points, horizon) is the window of a path on either side.
//   clear_a[i]     <=> fv_a[i] == w_a[i]          (k_select_audit's first violation; side B alike, or true for tracks)
//   feasible(i, j) <=> clear_a[i] && clear_b[j] && clearance(i, j) >= pair_margin          (false for a NaN clearance)
//   S(i, j)         =  cost_a[i] + cost_b[j]       (one rounded add; tracks: track_cost[j], or +0.0)
//   g(i, j)         =  min(c_a[i] - obstacle_margin, c_b[j] - obstacle_margin, clearance(i, j) - pair_margin), each one
//                      rounded subtraction, the minimum by `<` in that order (tracks: no c_b term)
//   m               =  the feasible pair of least S, strict `<` from +inf in row-major order
//   rule 0 keep prev / 1 m / 2 the pair of greatest g among the pairs with a non-NaN clearance term / -1 none
//
// k_pairclear_window   the windowed lengths min(n_points, horizon) of both sides into scratch: k_cross_audit[_slack]
//                      read their CrossAuditArgs::len_a / len_b from there and so audit the paths cut to their windows
//                      without a change to either kernel.
// k_pairclear_reduce   up to PMAF_XAUDIT_PARTIALS blocks of 256 threads grid-stride over the N_a * N_b pairs in ascending
//                      index; a pair reads one double of the matrix and, per side, cost, c, fv and w of its member (rows
//                      and columns of the matrix: cache hits). A thread carries
//                        - the least feasible (S, idx): strict `<` over ascending idx, so the smallest idx of its best S,
//                        - the greatest (g, -idx) over the pairs that take part, carried as the least (-g, idx),
//                        - the integer count of feasible pairs.
//                      group_argmin butterflies, then LDS across the four waves (k_pair_reduce's structure).
// k_pairclear_final    one block folds the partials the same way, counts the clear agents of both sides (integer
//                      sums), applies the rule -- the reads of prev_pair's feasibility and sum included --, writes the
//                      result record into mapped pinned host memory behind a sequence number (as k_select_pick) and,
//                      when asked, performs the adopt stores (adopt_agent, pmaf_adopt.hpp: wave 0 for side A, wave 1
//                      for side B).
// Every reduction is a minimum under a total order -- (S, idx) and (-g, idx): a NaN never enters either, idx breaks every
// tie -- or an integer sum: exact, associative and commutative, so the result does not depend on the grid, on the split
// over waves or on the butterflies' order. It is what the row-major strict scans of the contract find. No atomics, no
// last-block-done counter: the launches are ordered by the stream.
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_adopt.hpp"

using namespace pmaf;

#define PMAF_PAIRCLEAR_THREADS 256
#define PMAF_PAIRCLEAR_NONE 0x7fffffff

__global__ __launch_bounds__(PMAF_PAIRCLEAR_THREADS) void k_pairclear_window(PairWindowArgs A) {
  const int t = blockIdx.x * PMAF_PAIRCLEAR_THREADS + threadIdx.x;
  if (t >= A.count_a + A.count_b) return;
  const bool is_b = t >= A.count_a;
  const int e = is_b ? t - A.count_a : t;
  int n = (is_b ? A.n_b : A.n_a)[e];
  PMAF_BOUND(n >= 0 && n <= A.cap);
  n = n < A.cap ? n : A.cap;
  n = n > 0 ? n : 0;
  (is_b ? A.len_b : A.len_a)[e] = n < A.horizon ? n : A.horizon;
}

// what one pair contributes: feasibility, sum and worst excess, in the contract's operations
struct PairTerms {
  double s, g, clearance;
  bool feasible, takes_part;
};

__device__ __forceinline__ PairTerms pair_terms(const PairClearArgs &A, int i, int j) {
  PairTerms t;
  t.clearance = A.clearance[(size_t)i * A.n_b + j];
  const bool clear_a = A.fv_a[i] == A.len_a[i];
  const bool clear_b = A.fv_b ? A.fv_b[j] == A.len_b[j] : true;
  t.s = A.cost_a[i] + (A.cost_b ? A.cost_b[j] : 0.0);
  t.feasible = clear_a && clear_b && t.clearance >= A.pair_margin;
  double g = A.clr_a[i] - A.obstacle_margin;
  if (A.clr_b) {
    const double gb = A.clr_b[j] - A.obstacle_margin;
    if (gb < g) g = gb;
  }
  const double gp = t.clearance - A.pair_margin;
  if (gp < g) g = gp;
  t.g = g;
  t.takes_part = !(gp != gp);
  return t;
}

__device__ __forceinline__ void pairclear_fold(PairClearBest &b, double s, int si, double ng, int gi, int nfeas) {
  const bool ts = (s < b.s) || (s == b.s && si < b.si);
  b.s = ts ? s : b.s;
  b.si = ts ? si : b.si;
  const bool tg = (ng < b.ng) || (ng == b.ng && gi < b.gi);
  b.ng = tg ? ng : b.ng;
  b.gi = tg ? gi : b.gi;
  b.nfeas += nfeas;
}

// over the block's threads; the result is valid in thread 0
__device__ __forceinline__ void pairclear_block_reduce(PairClearBest &b) {
  constexpr int W = PMAF_PAIRCLEAR_THREADS / 64;
  __shared__ double s_s[W], s_g[W];
  __shared__ int s_si[W], s_gi[W], s_nf[W];
  group_argmin<64>(b.s, b.si);
  group_argmin<64>(b.ng, b.gi);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) b.nfeas += __shfl_xor(b.nfeas, off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_s[wave] = b.s; s_si[wave] = b.si; s_g[wave] = b.ng; s_gi[wave] = b.gi; s_nf[wave] = b.nfeas; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < W; w++) pairclear_fold(b, s_s[w], s_si[w], s_g[w], s_gi[w], s_nf[w]);
}

__global__ __launch_bounds__(PMAF_PAIRCLEAR_THREADS) void k_pairclear_reduce(PairClearArgs A) {
  const double inf = __builtin_huge_val();
  PairClearBest b{inf, inf, PMAF_PAIRCLEAR_NONE, PMAF_PAIRCLEAR_NONE, 0, 0};
  const int total = A.n_a * A.n_b;
  // ascending indices per thread and strict comparisons: a thread keeps the smallest index of its best value
  for (int idx = blockIdx.x * PMAF_PAIRCLEAR_THREADS + threadIdx.x; idx < total;
       idx += gridDim.x * PMAF_PAIRCLEAR_THREADS) {
    const int i = idx / A.n_b, j = idx - i * A.n_b;
    const PairTerms t = pair_terms(A, i, j);
    b.nfeas += t.feasible ? 1 : 0;
    if (t.feasible && t.s < b.s) { b.s = t.s; b.si = idx; }              // false for a NaN sum and a sum of +inf
    if (t.takes_part && -t.g < b.ng) { b.ng = -t.g; b.gi = idx; }        // g > running maximum, from -inf
  }
  pairclear_block_reduce(b);
  if (threadIdx.x == 0) A.partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(PMAF_PAIRCLEAR_THREADS) void k_pairclear_final(DevView D, PairClearArgs A, int n_partials) {
  __shared__ int s_n[2][PMAF_PAIRCLEAR_THREADS / 64];
  __shared__ int s_pick[2];
  const double inf = __builtin_huge_val();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  PairClearBest b{inf, inf, PMAF_PAIRCLEAR_NONE, PMAF_PAIRCLEAR_NONE, 0, 0};
  if ((int)threadIdx.x < n_partials) b = A.partial[threadIdx.x];
  pairclear_block_reduce(b);
  // the clear agents of both sides (tracks: every track counts)
  int nc_a = 0, nc_b = 0;
  for (int i = threadIdx.x; i < A.n_a; i += PMAF_PAIRCLEAR_THREADS) nc_a += A.fv_a[i] == A.len_a[i] ? 1 : 0;
  for (int j = threadIdx.x; j < A.n_b; j += PMAF_PAIRCLEAR_THREADS) nc_b += (A.fv_b ? A.fv_b[j] == A.len_b[j] : true) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nc_a += __shfl_xor(nc_a, off);
    nc_b += __shfl_xor(nc_b, off);
  }
  if (lane == 0) { s_n[0][wave] = nc_a; s_n[1][wave] = nc_b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < PMAF_PAIRCLEAR_THREADS / 64; w++) { nc_a += s_n[0][w]; nc_b += s_n[1][w]; }
    int idx, rule;
    if (b.si != PMAF_PAIRCLEAR_NONE) {
      idx = b.si;
      rule = 1;
      PMAF_BOUND(A.prev_i >= -1 && A.prev_i < A.n_a && A.prev_j >= -1 && A.prev_j < A.n_b);
      if (A.prev_i >= 0 && A.prev_i < A.n_a && A.prev_j >= 0 && A.prev_j < A.n_b) {
        const PairTerms q = pair_terms(A, A.prev_i, A.prev_j);
        // evaluateAgents' hysteresis (B/src/cf_manager.cpp:344-350) on the feasible set; a NaN sum of prev fails the `>=`
        if (q.feasible && b.s >= 0.9 * q.s) { idx = A.prev_i * A.n_b + A.prev_j; rule = 0; }
      }
    } else if (b.gi != PMAF_PAIRCLEAR_NONE) {
      idx = b.gi;
      rule = 2;
    } else {
      idx = -1;
      rule = -1;
    }
    double *r = A.result;
    const double nan = __builtin_nan("");
    r[2] = (double)rule;
    r[3] = (double)b.nfeas;
    r[4] = (double)nc_a;
    r[5] = (double)nc_b;
    if (idx >= 0) {
      PMAF_BOUND(idx < A.n_a * A.n_b);
      const int i = idx / A.n_b, j = idx - i * A.n_b;
      const PairTerms t = pair_terms(A, i, j);
      r[0] = (double)i;
      r[1] = (double)j;
      r[6] = t.s;
      r[7] = t.clearance;
      r[8] = A.clr_a[i];
      r[9] = A.clr_b ? A.clr_b[j] : inf;
      r[10] = (double)A.fv_a[i];
      r[11] = (double)(A.fv_b ? A.fv_b[j] : A.len_b[j]);
      r[12] = t.g;
      const int sa = A.step_a ? A.step_a[idx] : -1;
      r[13] = (double)sa;
      r[14] = (double)(A.step_b ? A.step_b[idx] : sa);
      s_pick[0] = i;
      s_pick[1] = j;
    } else {
      r[0] = r[1] = -1.0;
      r[6] = r[7] = r[8] = r[9] = r[12] = nan;
      r[10] = r[11] = r[13] = r[14] = -1.0;
      s_pick[0] = s_pick[1] = -1;
    }
  }
  __syncthreads();
  if (A.adopt && s_pick[0] >= 0) {
    if (wave == 0) adopt_agent(D, A.pop_a, s_pick[0], lane);
    if (wave == 1 && A.pop_b >= 0) adopt_agent(D, A.pop_b, s_pick[1], lane);
  }
  __threadfence_system();   // the record and the adopt stores before the sequence number
  __syncthreads();
  if (threadIdx.x == 0) *reinterpret_cast<volatile double *>(A.result + PMAF_PAIRCLEAR_REC - 1) = A.seq;
}

void pmaf_k_launch_pairclear_window(const PairWindowArgs &A, hipStream_t s) {
  const int total = A.count_a + A.count_b;
  hipLaunchKernelGGL(k_pairclear_window, dim3((unsigned)((total + PMAF_PAIRCLEAR_THREADS - 1) / PMAF_PAIRCLEAR_THREADS)),
                     dim3(PMAF_PAIRCLEAR_THREADS), 0, s, A);
}

void pmaf_k_launch_pairclear(const DevView &D, const PairClearArgs &A, hipStream_t s) {
  const int total = A.n_a * A.n_b;
  int blocks = (total + PMAF_PAIRCLEAR_THREADS - 1) / PMAF_PAIRCLEAR_THREADS;
  blocks = blocks < PMAF_XAUDIT_PARTIALS ? blocks : PMAF_XAUDIT_PARTIALS;
  blocks = blocks > 0 ? blocks : 1;
  hipLaunchKernelGGL(k_pairclear_reduce, dim3((unsigned)blocks), dim3(PMAF_PAIRCLEAR_THREADS), 0, s, A);
  hipLaunchKernelGGL(k_pairclear_final, dim3(1), dim3(PMAF_PAIRCLEAR_THREADS), 0, s, D, A, blocks);
}
