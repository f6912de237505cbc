// pmaf_auditft.hpp -- the audits against the obstacle tracks (include/pmaf.h "audits against the obstacle tracks"):
// the launch interface between pmaf_host_audit.cpp and pmaf_k_auditft.hip, and the launcher of k_path_audit alone that
// the tracked path audit needs (stage and pick have launchers of their own in pmaf_types.hpp). A header of its own so that no other kernel unit's inputs change with
// it: DevView, SelectArgs and AuditArgs stay what they are, and the tracks travel as pmaf_ftrack.hpp's FTrackArgs.
#pragma once
#include "pmaf_types.hpp"
#include "pmaf_ftrack.hpp"

// FTrackArgs as the audits read it: pts / len / max_len are the handle's resident buffers (what the next rollout launch
// would follow), first is the handle's device array or the call's own offsets in mapped pinned host memory. Population p
// with L = len[p] > 0 has its field obstacle j < M = n_obs - 1 at the position of point min(min(first[p], L-1) + k, L-1)
// at step k; the trailing obstacle j = M, and every obstacle of a population with L == 0, walks the list's chain.

// pmaf_k_auditft.hip: k_ft_select_audit on grid (N, P) -- k_select_audit's outputs (A.clr, A.fv) for a tracked handle;
// with cols != NULL k_ft_masked_audit, the same with the audited columns of two populations given as masks
// (pmaf_xattach.hpp). The list must already be staged (pmaf_k_launch_select_stage). Needs D.n_obs <= 64 (a tracked
// handle has <= 61).
struct AuditColumns;
void pmaf_k_launch_select_audit_ft(const DevView &D, const SelectArgs &A, const FTrackArgs &F, const AuditColumns *cols,
                                   hipStream_t s);
// pmaf_k_auditft.hip: k_audit_track_ft -- k_audit_track's buffer track [P][cap][3][n_obs] with the tracked columns
void pmaf_k_launch_audit_track_ft(const DevView &D, const double *obs, const FTrackArgs &F, double *track, hipStream_t s);
// pmaf_k_misc.hip: k_path_audit alone, on a track buffer that is already built (A.track)
void pmaf_k_launch_path_audit_only(const DevView &D, const AuditArgs &A, hipStream_t s);
