// pmaf_xattach.hpp -- the cross audit on coupled handles (include/pmaf.h "joint selection on coupled handles":
// pmaf_cross_audit_attached, pmaf_select_pair_clear_tracked, and their slacked forms): the structs and the launch interface
// between pmaf_host_audit.cpp and the kernels the calls add -- k_cross_audit_attached (pmaf_k_xattach.hip),
// k_xaudit_attached_slack (pmaf_k_xattach_slack.hip) and k_ft_masked_audit (pmaf_k_auditft.hip). A header of its own so that no other kernel unit's inputs change with it:
// CrossAuditArgs, SelectArgs and FTrackArgs stay what they are. Read by the host compiler too: the device code of the terms
// is in pmaf_xattach_terms.hpp.
#pragma once
#include "pmaf_types.hpp"
#include "pmaf_ftrack.hpp"

// The terms of a pair beside the end effectors: the spheres of one population's list that ride on the OTHER population's
// candidate path. All of it is the coupling's resident state (pmaf_fcouple.hpp: FCoupleArgs::src / scale / anchor, the
// rows of the two populations) and the staged list's radii; nothing is uploaded for a call.
//   term 0            x against y, R = separation
//   term 1 + s        src_a[s] == pop_b: x against anchor_a[s] + scale_a[s] * y, R = radius + rad_a[s]
//   term 1 + M + s    src_b[s] == pop_a: y against anchor_b[s] + scale_b[s] * x, R = radius + rad_b[s]
struct XAttachSide {
  const int32_t *src;       // [64] the population's row of FCoupleArgs::src, or NULL: nothing attached
  const double *scale;      // [64]
  const double *anchor;     // [3][64]
  const double *rad;        // [M] the radii of the population's staged list (row 6 of its [7][n_obs] block)
};
struct CrossAuditAttachedArgs {
  CrossAuditArgs X;         // the two sets, separation, clearance and step as in the cross audit
  XAttachSide a, b;         // the lists of pop_a and of pop_b
  int pop_a, pop_b, M;      // M = n_obs - 1 <= 60 while anything is attached
  double radius;            // pmaf_params.radius
  int32_t *sphere;          // [n_a][n_b] or NULL: the winning term's code
};

// pmaf_k_xattach.hip: k_cross_audit_attached on the cross audit's grid
void pmaf_k_launch_cross_audit_attached(const CrossAuditAttachedArgs &A, hipStream_t s);

// the attached audit with timing slack (include/pmaf.h "joint selection on coupled handles with timing slack":
// pmaf_cross_audit_attached_slack, pmaf_select_pair_clear_tracked_slack): the terms above, every term over the slacked
// audit's band. k is A's step and l B's in every term: T.X.step = step_a.
struct CrossAuditAttachedSlackArgs {
  CrossAuditAttachedArgs T;
  int32_t *step_b;          // [n_a][n_b] or NULL
  int late_a, late_b;       // 0 .. cap each (clamped on the host): admitted (k, l) iff -late_b <= l - k <= late_a
};

// pmaf_k_xattach_slack.hip: k_xaudit_attached_slack on the cross audit's grid
void pmaf_k_launch_cross_audit_attached_slack(const CrossAuditAttachedSlackArgs &A, hipStream_t s);

// the obstacle side's audited columns of the joint selection's two populations: bit j set = obstacle j of the list is
// audited. Every other population of the handle keeps columns 0 .. SelectArgs::n_audit - 1. Handed to the tracked audit's
// launcher (pmaf_k_launch_select_audit_ft, pmaf_auditft.hpp), which then runs k_ft_masked_audit.
struct AuditColumns {
  int pop_a, pop_b;
  unsigned long long cols_a, cols_b;
};
