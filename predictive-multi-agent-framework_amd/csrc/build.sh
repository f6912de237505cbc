#!/bin/bash
# Builds libpmaf_hip.so (HIP kernels + C-ABI) for gfx950, in-tree.
#
# Translation units (compiled in parallel, objects kept in ../lib/obj):
#   pmaf_k_w64.hip   x5  the wave-per-agent rollout kernel, once per arithmetic policy (-DPMAF_W64_MATH=0|1|2|3; the default
#                        policy 2 in two units: one-slot / multi-slot kernels, -DPMAF_W64_PART=1|2; policy 3 = the opt-in
#                        contracted one, the only units compiled with -ffp-contract=fast). The step (rollout_w64_body) and
#                        its dispatch live in the header pmaf_rollout_w64_body.hpp, which the two track units include too
#                        (the text of one step in pmaf_rollout_w64_step.hpp: the body includes it once per step loop)
#   pmaf_k_grp.hip   x3  the group rollout kernel (-DPMAF_GRP_MATH=0|2|3)
#   pmaf_k_mw.hip    x3  the multi-wave-per-agent rollout kernel (62..256 obstacles at <= 1 wave per SIMD; -DPMAF_MW_MATH=1|2|3)
#   pmaf_k_misc.hip      generic rollout, manager, scoring, winner records, the path audit (pmaf_path_audit.hpp), the cross audit (pmaf_xaudit_kernels.hpp) ... + the launch interface
#   pmaf_k_slack.hip     the cross audit with timing slack (k_cross_audit_slack: the band walk of the tile header
#                        pmaf_cross_audit.hpp, which all four cross-audit kernels -- this one, k_cross_audit in
#                        pmaf_k_misc.hip and the two attached units below -- include), a unit of its own so that the other units'
#                        code objects do not move with it; its object is slack.o, outside the k_*.o set of twelve whose
#                        disassembly tests/test_abi.py walks (tests/test_slack_audit.py holds it to the same: no scratch)
#   pmaf_k_select.hip    the selection against the live list (pmaf_select_clear / pmaf_adopt_best), a unit of its own for
#                        the same reason; its object is select.o, outside the k_*.o set like slack.o; k_select_audit is an
#                        instance of pmaf_select_audit.hpp's one body, like the two audits of pmaf_k_auditft.hip
#                        (tests/test_select_clear.py holds its kernels to no scratch through the resource record)
#   pmaf_k_pairclear.hip the joint selection (pmaf_select_pair_clear / pmaf_select_clear_tracks): the windowed lengths, the
#                        joint reduction and its final block; a unit of its own for the same reason, object pairclear.o
#                        (tests/test_pair_clear.py holds its kernels to no scratch through the resource record)
#   pmaf_k_track.hip     the repulsive track (include/pmaf.h): k_rollout_w64_track -- the one-slot wave-per-agent body of
#                        pmaf_rollout_w64_body.hpp instantiated with the tracked obstacle, compiled with the one-slot unit's flags --
#                        and k_track_from_best; a unit of its own for the same reason, object track.o
#                        (tests/test_sentinel_track.py holds its kernels to no scratch through the resource record)
#   pmaf_k_ftrack.hip    the obstacle tracks (include/pmaf.h): k_rollout_w64_ftrack -- the same body instantiated with the
#                        tracked field obstacles (and the tracked trailing one), compiled with the one-slot unit's flags;
#                        a unit of its own for the same reason, object ftrack.o
#                        (tests/test_field_track.py holds its kernels to no scratch through the resource record)
#   pmaf_k_auditft.hip   the audits against the obstacle tracks (pmaf_select_clear_tracked / pmaf_evaluate_paths_tracked):
#                        k_ft_select_audit, k_ft_masked_audit (pmaf_select_audit.hpp's body) and k_audit_track_ft (the chain of
#                        pmaf_audit_chain.hpp), compiled with select.o's flags; a unit of its own for the
#                        same reason, object auditft.o
#                        (tests/test_tracked_audit.py holds its kernels to no scratch through the resource record)
#   pmaf_k_fcouple.hip   the obstacle tracks' device-side source (pmaf_couple_obstacle_tracks): k_fcouple_take and
#                        k_fcouple_compose, compiled with the plain kernel flags (-ffp-contract=off: the composed
#                        position is one rounded multiply and one rounded add); a unit of its own for the same reason,
#                        object fcouple.o
#                        (tests/test_field_couple.py holds its kernels to no scratch through the resource record)
#   pmaf_k_ftingest.hip  the obstacle tracks' device-memory source (pmaf_set_obstacle_tracks_device): k_ftingest_check and
#                        k_ftingest_store, each for double | float elements and 6 | 3 components, compiled with the plain
#                        kernel flags (-ffp-contract=off, as fcouple.o: the derived velocity is one rounded difference
#                        and one rounded quotient); a unit of its own for the same reason, object ftingest.o
#                        (tests/test_track_ingest.py holds its kernels to no scratch through the resource record)
#   pmaf_k_xattach.hip   the cross audit on coupled handles (pmaf_cross_audit_attached / pmaf_select_pair_clear_tracked):
#                        k_cross_audit_attached, the step walk of the tile header pmaf_cross_audit.hpp over the terms of
#                        pmaf_xattach_terms.hpp (device only; shared with the next unit), compiled with the plain kernel
#                        flags (-ffp-contract=off: the riding sphere is one rounded multiply and one rounded add); a unit
#                        of its own for the same reason, object xattach.o
#                        (tests/test_attached_audit.py holds its kernel to no scratch through the resource record)
#   pmaf_k_xattach_slack.hip the attached audit with timing slack (pmaf_cross_audit_attached_slack /
#                        pmaf_select_pair_clear_tracked_slack): k_xaudit_attached_slack, the same two headers: the
#                        attached audit's terms over the tile header's band walk, compiled with the plain kernel flags
#                        (-ffp-contract=off, as xattach.o); a unit of its own for the same reason, object xattach_slack.o
#                        (tests/test_attached_slack_audit.py holds its kernel to no scratch through the resource record)
#   pmaf_k_obslack.hip   the audits against the live list with timing slack (pmaf_evaluate_paths_slack /
#                        pmaf_select_clear_slack): k_obs_slack_audit<false|true>, the body of pmaf_obstacle_slack.hpp (which
#                        takes ft_window from pmaf_select_audit.hpp), compiled with the plain kernel flags
#                        (-ffp-contract=off, as auditft.o); a unit of its own for the same reason, object obslack.o,
#                        outside the k_*.o set like slack.o
#                        (tests/test_obstacle_slack_audit.py holds its kernels to no scratch through the resource record)
#   pmaf_k_dbgmath.hip   ops 13..20 of pmaf_debug_math (test support: the policies' elementary operations that ops 0..12 in
#                        pmaf_k_misc.hip do not reach), a unit of its own for the same reason; its object is dbgmath.o
#   pmaf_host.cpp        the C-ABI (g++, plain C++ against the HIP runtime API): handle, tick protocol, repulsive track,
#                        stepping API, getters; with three units of its own for what pmaf_tick does not run --
#   pmaf_host_audit.cpp    the path audit, the selections, the cross audit, the link force
#   pmaf_host_exchange.cpp the winner-record exchange and the peer mailboxes
#   pmaf_host_state.cpp    checkpointing
#                        (they share pmaf_host_impl.hpp: the handle, its owning buffers, the bounded wait; host units only,
#                        not in DEPS_K; the host objects are compiled on every build)
#   pmaf_shard.cpp       communicators + the winner-record exchange (RCCL / host-callback)
# linked with -lamdhip64 -lrccl.
#
# -ffp-contract=off: no FMA contraction, so the kernels keep the reference's
# double-precision operation order (see pmaf_device.hpp).
# -amdgpu-sched-strategy=max-ilp: the rollout waves run one or two per SIMD, so
# the machine scheduler should interleave the independent sqrt / divide chains
# rather than protect an occupancy these kernels never reach (measured: C2
# 403 -> 382 us, C3 1974 -> 1751 us, C5 1128 -> 1096 us per tick kernel).
set -e
cd "$(dirname "$0")"
ROCM=${ROCM_PATH:-/opt/rocm}
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
CXX=${CXX:-g++}
# PMAF_VARIANT: a second product library with another EVALUATION-ORDER policy, built into ../lib_<variant>/ --
#   rassoc   3-vector dot products / squared norms associate as a0 b0 + (a1 b1 + a2 b2): Eigen 3.3's NON-vectorised
#            redux (EIGEN_DONT_VECTORIZE, targets without a double-precision packet type) instead of the default
#            (a0 b0 + a1 b1) + a2 b2 of its SSE2 / NEON packet path (Redux.h: predux of the first packet, then the
#            remaining coefficient). -DPMAF_DOT_RIGHT_ASSOC on kernels AND host; the oracle has the same switch
#            (oracle/pmaf_oracle.c) and the 0-tolerance suite runs against either pair (tests/test_build_variants.py).
#            pmaf_eval_order() reports which one a library was built with.
case "${PMAF_VARIANT:-}" in
  "") ;;
  rassoc) PMAF_OUT=${PMAF_OUT:-../lib_rassoc}; PMAF_EXTRA_FLAGS="$PMAF_EXTRA_FLAGS -DPMAF_DOT_RIGHT_ASSOC" ;;
  *) echo "build.sh: unknown PMAF_VARIANT '$PMAF_VARIANT' (known: rassoc)" >&2; exit 2 ;;
esac
OUT=${PMAF_OUT:-../lib}   # PMAF_OUT: another output directory (variant / timer builds under tools/dbg)
OBJ=$OUT/obj
mkdir -p "$OBJ"
# -Rpass-analysis=kernel-resource-usage: registers / occupancy of every kernel,
# kept next to the library. The group kernel's throughput rests on TWO waves per
# SIMD (<= 256 VGPRs; it sits at ~252, and one innocent-looking variant landed
# on 268: occupancy 1, +50 % time), so tests/test_abi.py checks the record.
KFLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -mllvm -amdgpu-sched-strategy=max-ilp -mllvm -amdgpu-atomic-optimizer-strategy=None \
  -Wall -Wno-unused-function -Rpass-analysis=kernel-resource-usage ${PMAF_EXTRA_FLAGS} ${PMAF_EXTRA_KFLAGS}"   # PMAF_EXTRA_KFLAGS: kernel objects only
# PMAF_EXTRA_HFLAGS / PMAF_EXTRA_LDFLAGS: host objects / link line only (sanitizer builds: tools/asan.sh)
HFLAGS="-O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -D__HIP_PLATFORM_AMD__ -I$ROCM/include ${PMAF_EXTRA_FLAGS} ${PMAF_EXTRA_HFLAGS}"

DEPS_K="pmaf_types.hpp pmaf_device.hpp pmaf_rollout_w64.hpp pmaf_rollout_w64_body.hpp pmaf_rollout_w64_step.hpp pmaf_rollout_grp.hpp pmaf_path_audit.hpp pmaf_xaudit_kernels.hpp pmaf_cross_audit.hpp pmaf_adopt.hpp"
DEPS_TRACK="pmaf_track.hpp"   # what pmaf_k_track.hip includes beside DEPS_K
DEPS_FTRACK="pmaf_track.hpp pmaf_ftrack.hpp"   # ... and pmaf_k_ftrack.hip
DEPS_SELECT="pmaf_track.hpp pmaf_ftrack.hpp pmaf_select_audit.hpp"   # ... and pmaf_k_select.hip
DEPS_AUDITFT="$DEPS_SELECT pmaf_audit_chain.hpp pmaf_auditft.hpp pmaf_xattach.hpp"   # ... and pmaf_k_auditft.hip
DEPS_XATTACH="pmaf_ftrack.hpp pmaf_xattach.hpp pmaf_xattach_terms.hpp"   # ... and pmaf_k_xattach.hip
DEPS_XATTACH_SLACK="pmaf_ftrack.hpp pmaf_xattach.hpp pmaf_xattach_terms.hpp"   # ... and pmaf_k_xattach_slack.hip
DEPS_OBSLACK="$DEPS_SELECT pmaf_obstacle_slack.hpp"   # ... and pmaf_k_obslack.hip
DEPS_FCOUPLE="pmaf_track.hpp pmaf_ftrack.hpp pmaf_fcouple.hpp"   # ... and pmaf_k_fcouple.hip
DEPS_FTINGEST="pmaf_track.hpp pmaf_ftrack.hpp pmaf_ftingest.hpp ../../include/pmaf.h"   # ... and pmaf_k_ftingest.hip
# the objects of an output directory belong to ONE set of flags: a directory built with other flags is rebuilt
STAMP="$KFLAGS | $HFLAGS | $PMAF_EXTRA_LDFLAGS"
FLAGS_CHANGED=0
[ "$(cat "$OBJ/flags.txt" 2>/dev/null)" = "$STAMP" ] || FLAGS_CHANGED=1
pids=()
names=()
kcompile() {  # kcompile <object stem> <source> [defines...]
  local stem=$1 src=$2; shift 2
  local o="$OBJ/$stem.o"
  local stale=0
  [ -f "$o" ] || stale=1
  local extra=""
  [ "$src" = pmaf_k_track.hip ] && extra=$DEPS_TRACK
  [ "$src" = pmaf_k_ftrack.hip ] && extra=$DEPS_FTRACK
  [ "$src" = pmaf_k_select.hip ] && extra=$DEPS_SELECT
  [ "$src" = pmaf_k_auditft.hip ] && extra=$DEPS_AUDITFT
  [ "$src" = pmaf_k_fcouple.hip ] && extra=$DEPS_FCOUPLE
  [ "$src" = pmaf_k_ftingest.hip ] && extra=$DEPS_FTINGEST
  [ "$src" = pmaf_k_obslack.hip ] && extra=$DEPS_OBSLACK
  [ "$src" = pmaf_k_xattach.hip ] && extra=$DEPS_XATTACH
  [ "$src" = pmaf_k_xattach_slack.hip ] && extra=$DEPS_XATTACH_SLACK
  for d in $src $DEPS_K $extra build.sh; do [ "$d" -nt "$o" ] && stale=1; done
  [ "$FLAGS_CHANGED" = 1 ] && stale=1
  [ "$stale" = 0 ] && return 0
  ( $HIPCC $KFLAGS "$@" -c "$src" -o "$o" 2> "$OBJ/$stem.log" ) &
  pids+=($!); names+=("$stem")
}
# default policy: one-slot and multi-slot kernels in units of their own -- the multi-slot kernels (C3) are 2.4 % faster
# with top-down pre-RA scheduling (1080 -> 1054 us per launch), the one-slot kernels (C1, C2) 1 % slower (one box,
# tools/dbg/ab variants; profiles/r3_ab_sched_flags.txt)
# (last session of round 4: loops aligned to 32 bytes in this unit -- with the repulsive obstacle's rider the unaligned layout
# cost C1 0.9 % and C2 0.5 %, aligned 0.0 / 0.4 %, and C4 gains another 0.9 %: profiles/r4_ab_w64.txt item 8)
# (round 5, with the glibc-compatible exp and its table load in the scaling chain: -DPMAF_SUM_TAIL_PIN=1 keeps that chain's
# tail in the block of the ordered sum's first chunk -- C1 110.2 -> 108.7, C2 226.0 -> 224.3 us on one box)
kcompile k_w64_m2_t1 pmaf_k_w64.hip -DPMAF_W64_MATH=2 -DPMAF_W64_PART=1 -falign-loops=32 -DPMAF_SUM_TAIL_PIN=1
# (third session: and with every block that is not fallen into aligned to 64 bytes -- C3 1018.9 -> 1011.2 us on one box, any
# alignment from 16 to 128 bytes within 2 us of that; the one-slot kernels lose 0.2-0.8 % with it, the group kernel is
# indifferent: profiles/r3_ab_session3.txt item 19)
kcompile k_w64_m2_tn pmaf_k_w64.hip -DPMAF_W64_MATH=2 -DPMAF_W64_PART=2 -mllvm -misched-prera-direction=topdown -mllvm -align-all-nofallthru-blocks=6
kcompile k_w64_m0 pmaf_k_w64.hip -DPMAF_W64_MATH=0
kcompile k_w64_m1 pmaf_k_w64.hip -DPMAF_W64_MATH=1
kcompile k_grp_m2 pmaf_k_grp.hip -DPMAF_GRP_MATH=2
# contracted policy (PMAF_FLAG_CONTRACTED, opt-in; tolerance parity): the only units built with FMA contraction
kcompile k_w64_m3 pmaf_k_w64.hip -DPMAF_W64_MATH=3 -ffp-contract=fast
kcompile k_grp_m3 pmaf_k_grp.hip -DPMAF_GRP_MATH=3 -ffp-contract=fast
kcompile k_grp_m0 pmaf_k_grp.hip -DPMAF_GRP_MATH=0
kcompile k_mw_m2 pmaf_k_mw.hip -DPMAF_MW_MATH=2
kcompile k_mw_m1 pmaf_k_mw.hip -DPMAF_MW_MATH=1
kcompile k_mw_m3 pmaf_k_mw.hip -DPMAF_MW_MATH=3 -ffp-contract=fast
kcompile k_misc pmaf_k_misc.hip
kcompile slack pmaf_k_slack.hip
kcompile select pmaf_k_select.hip
kcompile pairclear pmaf_k_pairclear.hip
kcompile auditft pmaf_k_auditft.hip
kcompile dbgmath pmaf_k_dbgmath.hip
kcompile fcouple pmaf_k_fcouple.hip
kcompile ftingest pmaf_k_ftingest.hip
kcompile xattach pmaf_k_xattach.hip
kcompile xattach_slack pmaf_k_xattach_slack.hip
kcompile obslack pmaf_k_obslack.hip
# (the flags of k_w64_m2_t1: the same body)
kcompile track pmaf_k_track.hip -DPMAF_W64_MATH=2 -falign-loops=32 -DPMAF_SUM_TAIL_PIN=1
kcompile ftrack pmaf_k_ftrack.hip -DPMAF_W64_MATH=2 -falign-loops=32 -DPMAF_SUM_TAIL_PIN=1
HOST_UNITS="host host_audit host_exchange host_state shard"   # pmaf_<unit>.cpp -> <unit>.o, all with HFLAGS
for u in $HOST_UNITS; do
  ( $CXX $HFLAGS -c "pmaf_$u.cpp" -o "$OBJ/$u.o" 2> "$OBJ/$u.log" ) &
  pids+=($!); names+=("$u")
done
fail=0
for i in "${!pids[@]}"; do
  if ! wait "${pids[$i]}"; then echo "compile failed: ${names[$i]}" >&2; cat "$OBJ/${names[$i]}.log" >&2; fail=1; fi
done
[ "$fail" = 0 ] || exit 1
printf '%s' "$STAMP" > "$OBJ/flags.txt"
for n in "${names[@]}"; do grep -E -A3 "warning:|error:" "$OBJ/$n.log" >&2 || true; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/libpmaf_hip.so" \
  "$OBJ"/k_w64_m2_t1.o "$OBJ"/k_w64_m2_tn.o "$OBJ"/k_w64_m0.o "$OBJ"/k_w64_m1.o "$OBJ"/k_grp_m2.o "$OBJ"/k_grp_m0.o "$OBJ"/k_w64_m3.o "$OBJ"/k_grp_m3.o "$OBJ"/k_mw_m1.o "$OBJ"/k_mw_m2.o "$OBJ"/k_mw_m3.o "$OBJ"/k_misc.o "$OBJ"/slack.o "$OBJ"/dbgmath.o "$OBJ"/select.o "$OBJ"/pairclear.o "$OBJ"/track.o "$OBJ"/ftrack.o "$OBJ"/auditft.o "$OBJ"/fcouple.o "$OBJ"/ftingest.o "$OBJ"/xattach.o "$OBJ"/xattach_slack.o "$OBJ"/obslack.o \
  $(for u in $HOST_UNITS; do echo "$OBJ/$u.o"; done) -L"$ROCM/lib" -lrccl -Wl,-rpath,"$ROCM/lib" ${PMAF_EXTRA_LDFLAGS}
# (the log of an object that was up to date is the one of its last compile)
cat "$OBJ"/k_*.log "$OBJ"/slack.log "$OBJ"/dbgmath.log "$OBJ"/select.log "$OBJ"/pairclear.log "$OBJ"/track.log "$OBJ"/ftrack.log "$OBJ"/auditft.log "$OBJ"/fcouple.log "$OBJ"/ftingest.log "$OBJ"/xattach.log "$OBJ"/xattach_slack.log "$OBJ"/obslack.log | grep "kernel-resource-usage" | sed -e 's/^[^ ]* remark: *//' -e 's/ \[-Rpass-analysis=kernel-resource-usage\]//' > "$OUT/resource_usage.txt"
echo "built $OUT/libpmaf_hip.so"
