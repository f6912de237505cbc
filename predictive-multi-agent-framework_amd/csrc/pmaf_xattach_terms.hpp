// pmaf_xattach_terms.hpp -- the attached audits' TERMS on the device: what k_cross_audit_attached (pmaf_k_xattach.hip)
// and k_xaudit_attached_slack (pmaf_k_xattach_slack.hip) share beside the tile and the walks of pmaf_cross_audit.hpp. A
// pair is held to several spheres (the contract: those units' headers, the structs: pmaf_xattach.hpp); a kernel walks
// the tile once per term and keeps, per pair, the least gap over the terms. Here: the loop over the terms, the functor that
// stages the sphere riding on a point, the fold of a finished term into a pair's running minimum, and the pair's store.
// Device code only, included by those two units (pmaf_xattach.hpp is read by the host compiler too).
#pragma once
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"
#include "pmaf_xattach.hpp"

namespace pmaf {

// what is staged of a path point. on: the sphere that rides on it -- one rounded multiply, one rounded add per component
// (the composer's formula, pmaf_k_fcouple.hip; the attached units are compiled without contraction); otherwise the point
// as it lies. `on` is block-uniform.
struct XAttachRide {
  bool on;
  double scale, ax, ay, az;
  __device__ __forceinline__ double operator()(double v, int c) const {
    if (!on) return v;
    // (values, not lvalues: the choice below must not become an address -- a conditional over the struct's members was
    // indexed in scratch)
    const double a0 = ax, a1 = ay, a2 = az;
    const double a = c == 0 ? a0 : (c == 1 ? a1 : a2);
    const double m = scale * v;
    return a + m;
  }
};

// the terms of a call, in order: body(t, fa, fb, R) once per term that exists -- term 0 and, while anything is attached,
// those of the 2 M candidate columns whose source is the other population (a block-uniform loop of integer compares; a
// handle without attachments runs term 0 alone). fa / fb: what is staged of a point of A / of B in the term, which
// tile carries the sphere: neither (term 0), B's (a column of A's list rides on y) or A's. A term's parameters are
// wave-uniform, read through uniform addresses from the coupling's rows and the staged list's radii, and kept as values.
// (The loop is here and the kernel's part is the body. A decode that the kernels call per term, with "skip" as its return
// value, was tried first: k_cross_audit_attached then took 89 SGPRs for 77 and 1 300 to 1 550 of its 1 163 disassembly
// lines differed from the parent's; in this form 90 differ, the record is the parent's. profiles/xaudit_shared_walks.md
// has the variants.)
template <typename Body>
__device__ __forceinline__ void xattach_for_each_term(const CrossAuditAttachedArgs &S, Body body) {
  const int M = S.M;
  PMAF_BOUND(M >= 0 && ((!S.a.src && !S.b.src) || M <= PMAF_FTRACK_LANES));
  const int n_terms = 1 + ((S.a.src || S.b.src) ? 2 * M : 0);
  for (int t = 0; t < n_terms; t++) {   // block-uniform, as is every branch on t
    bool on_a = false, on_b = false;
    double scale = 0.0, ax = 0.0, ay = 0.0, az = 0.0, R = S.X.separation;
    if (t > 0) {
      const bool of_a = t <= M;
      const int s = of_a ? t - 1 : t - 1 - M;
      const int32_t *src = of_a ? S.a.src : S.b.src;
      if (!src || src[s] != (of_a ? S.pop_b : S.pop_a)) continue;
      const double *anchor = of_a ? S.a.anchor : S.b.anchor;
      scale = (of_a ? S.a.scale : S.b.scale)[s];
      ax = anchor[s];
      ay = anchor[PMAF_FTRACK_LANES + s];
      az = anchor[2 * PMAF_FTRACK_LANES + s];
      on_b = of_a;
      on_a = !of_a;
      R = S.radius + (of_a ? S.a.rad : S.b.rad)[s];
    }
    body(t, XAttachRide{on_a, scale, ax, ay, az}, XAttachRide{on_b, scale, ax, ay, az}, R);
  }
}

// a pair's running minimum over the terms: the gap (root taken), the winning term's step(s) and its code. l is the
// slacked audit's step of B; the step-against-step kernel has none and never reads it.
struct XAttachBest {
  double gap = __builtin_huge_val();
  int k = -1, l = -1, t = -1;
  // term t's (d2, k, l) into the minimum: one sqrt per pair and term; strict, terms ascending -- ties keep the smallest
  // term. A term in which nothing won (every d2 NaN) has k = -1 and is not folded.
  __device__ __forceinline__ void fold(double d2, int tk, int tl, double R, int term) {
    const double g = __builtin_sqrt(d2) - R;
    const bool take = tk >= 0 && g < gap;
    gap = take ? g : gap;
    k = take ? tk : k;
    l = take ? tl : l;
    t = take ? term : t;
  }
};

// the store of pair (ti, tj) of the tile: xaudit_store_pair's conventions (the ragged edge is not stored; an empty path
// on either side, or nothing won: +inf / -1 / -1 [/ -1]), on a gap that already has its root taken. step_b: the slacked
// audit's second step matrix, or nullptr.
__device__ __forceinline__ void xattach_store_pair(const CrossAuditAttachedArgs &S, int a0, int b0, int ti, int tj,
                                                   const int *s_na, const int *s_nb, const XAttachBest &p, int32_t *step_b) {
  const CrossAuditArgs &A = S.X;
  const int i = a0 + ti, j = b0 + tj;
  if (i < A.n_a && j < A.n_b) {
    const bool won = p.k >= 0 && s_na[ti] > 0 && s_nb[tj] > 0;
    const size_t o = (size_t)i * A.n_b + j;
    A.clearance[o] = won ? p.gap : __builtin_huge_val();
    if (A.step) A.step[o] = won ? p.k : -1;
    if (step_b) step_b[o] = won ? p.l : -1;
    if (S.sphere) S.sphere[o] = won ? p.t : -1;
  }
}

}  // namespace pmaf
