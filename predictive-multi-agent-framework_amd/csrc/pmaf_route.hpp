// Which rollout kernel a handle launches, and with what: ONE pure function from everything the choice depends on
// (Input) to everything the host forwards (Route). Host-only like pmaf_lpa_model.hpp: no HIP call, no getenv, no handle;
// no kernel translation unit includes it. The handle (pmaf_host_impl.hpp) keeps an Input and the Route computed from it,
// and pmaf_host.cpp recomputes the Route (reroute) where an input changes: at create, where the gains / the mass enter the handle
// (refresh_plain_step), when an external kernel is loaded or unloaded, and when the multi-wave launcher refuses.
// tests/test_route.py drives this header alone (tests/cpp/route_table.cpp): the families, the boundaries of every rule
// and the invariants between the fields, without a device.
//
// The five families, in the order the rule tries them:
//   EXTERNAL        pmaf_debug_external_rollout: a kernel out of a code object file on the wave-per-agent grid (N x P)
//   MULTI_WAVE      k_rollout_mw (pmaf_k_mw.hip): 2 ... 4 waves per agent, 61 ... 256 field obstacles, a CU per block
//   WAVE_PER_AGENT  k_rollout_w64 / k_rollout_w64_sliced (pmaf_k_w64.hip): 64 lanes, 1 / 2 / 4 obstacle slots per lane
//   GROUP           k_rollout_grp (pmaf_k_grp.hip): 32 / 16 / 8 lanes per agent, 1 / 2 / 4 slots
//   GENERIC         k_rollout<LPA> (pmaf_k_misc.hip): any power-of-two mapping, any slot count
//
// Former homes, for comments in the kernel files that still cite them (those files are left as they are so that their
// objects stay byte-identical): pmaf_host.cpp's pick_lpa, pick_mw (pmaf_k_mw.hip's launcher names it), w64_sliced,
// pmaf_planner::uses_closest_table, launch_rollout's tiles64 ladder and pmaf_create's LDS sizing ("pmaf_host.cpp:
// lds_rollout" in pmaf_rollout_w64.hpp; "the host picks per launch" there is Route::dpp_sum) are all route() below.
#pragma once
#include <cstddef>

#include "pmaf_lpa_model.hpp"
#include "pmaf_types.hpp"

namespace pmaf_route {

enum Family : int { EXTERNAL = 0, MULTI_WAVE = 1, WAVE_PER_AGENT = 2, GROUP = 3, GENERIC = 4 };

struct Input {
  int N = 1, P = 1, M = 0;      // agents per population, populations, FIELD obstacles (the list without the trailing repulsive one)
  int n_simds = 1024;           // SIMDs of the device (4 per CU)
  int lanes_request = 0;        // pmaf_params::lanes_per_agent: 0 = choose (pick_lpa), else a power of two <= 64
  int math = pmaf::MATH_XACT;   // arithmetic policy of the handle (pmaf_device.hpp)
  bool plain_step = false;      // every k_attr != 0 and unit mass: the wave-per-agent kernels' PLAIN step (pmaf_k_w64.hip)
  bool external = false;        // pmaf_debug_external_rollout has a kernel loaded
  bool mw_refused = false;      // the multi-wave launcher refused this handle's launch once: the one-wave kernels from then on
  // the environment, as the host read it at create (tests, timing experiments)
  bool force_generic = false;   // PMAF_FORCE_GENERIC=1: always the generic k_rollout<LPA>
  int mw = -1;                  // PMAF_MW: 0 = one-wave kernels, 2 / 3 / 4 = that many waves; < 0: unset
  int mw_per = 0;               // PMAF_MW_PER: obstacles per wave (0: unset -- the even split)
  int mw_lds_kb = 0;            // PMAF_MW_LDS_KB: the multi-wave launcher's LDS request (0: its placement rule)
  bool dpp_sum = true;          // PMAF_SUM=dpp|lds: the one-slot wave-per-agent kernels' ordered force sum
  bool w64_slice = true;        // PMAF_W64_SLICE=0|1: the priority-slicing loop where the rule below offers it
  // a repulsive track is attached or the populations are coupled (include/pmaf.h "repulsive track"). It changes none of
  // the fields the rule decides -- a handle is never moved to another kernel family for its track --; Route::carries_track
  // says whether the launch the route names has the variant that follows one (pmaf_k_track.hip)
  bool tracked = false;
  // obstacle tracks are attached (include/pmaf.h "obstacle tracks"): likewise an input that moves no field the rule
  // decides; Route::carries_field_tracks says whether the routed launch exists as k_rollout_w64_ftrack (pmaf_k_ftrack.hip)
  bool field_tracked = false;
};

struct Route {
  Family family = GENERIC;
  int lpa = 64;                 // lanes per agent
  int slots = 1;                // obstacle slots per lane the routed one-wave kernel works through
  int tiles = 0;                // its TILES template value: 1 / 2 / 4 (0: the generic kernel, which loops at run time)
  int waves = 1, per = 0;       // MULTI_WAVE: waves per agent and field obstacles per wave; otherwise 1 and M
  int mw_lds_kb = 0;            // MULTI_WAVE: forwarded to the launcher
  bool sliced = false;          // WAVE_PER_AGENT: k_rollout_w64_sliced
  bool dpp_sum = true;          // WAVE_PER_AGENT: the ordered force sum of the one-slot kernels (two / four slots: always DPP)
  bool plain = false;           // WAVE_PER_AGENT, MULTI_WAVE: the PLAIN step
  int math = pmaf::MATH_XACT;   // the policy handed to the family's launcher
  bool closest_table = false;   // the closest-other table is kept current for this handle (k_manager, DevView::closest_idx)
  bool tuned_real_step = false; // ManagerArgs::tuned_real_step
  int n_blocks = 1;             // blocks per population of the GROUP / GENERIC grid (and of k_plan_steps)
  size_t lds_rollout = 0;       // dynamic LDS of the one-wave rollout launch (and of k_plan_steps), bytes
  bool carries_track = false;   // the routed launch exists as k_rollout_w64_track (whatever Input::tracked says)
  bool carries_field_tracks = false;   // ... and as k_rollout_w64_ftrack (whatever Input::field_tracked says)
};

static inline const char *family_name(Family f) {
  switch (f) {
    case EXTERNAL: return "external";
    case MULTI_WAVE: return "multi-wave";
    case WAVE_PER_AGENT: return "wave-per-agent";
    case GROUP: return "group";
    default: return "generic";
  }
}

// The mapping with the smallest estimated kernel time (pmaf_lpa_model.hpp: a table of measured launch times per
// mapping, obstacle slots per lane and waves per SIMD; profiles/r6_lpa_grid.txt). History of the rule it replaces:
// rounds 1-4 narrowed the mapping until the launch had <= 2048 waves (the wave per agent wins while every wave has a SIMD
// to itself and still at two per SIMD; the group kernels run best at two per SIMD); round 5 added "never more than two
// obstacle slots per lane in a narrower mapping" (profiles/r5_lpa_rule.txt: the three- / four-slot group bodies and the
// generic kernel cost more than another round of waves: 128 obstacles x 4096 agents 1882 -> 1149 us); round 6 measured
// the whole plane and found that rule 20 ... 31 % off in three regions (header of pmaf_lpa_model.hpp). BASELINE's
// configurations keep their mappings: C1-C4 the wave per agent, C5 x 8 on one GPU 16 lanes, x 4 32 lanes, x 2 / x 1 64.
// (pmaf_pick_lanes_per_agent exports exactly this function.)
static inline int pick_lpa(int N, int P, int M, int n_simds) {
  int lpa = pmaf_lpa::pick(N, P, M, n_simds);
  // known-flag bitmask holds 64 tiles per lane
  while ((M + lpa - 1) / lpa > 64 && lpa < 64) lpa *= 2;
  return lpa;
}

static inline Route route(const Input &in) {
  Route r;
  const int M = in.M;
  const long agents = (long)in.N * in.P;
  r.lpa = in.lanes_request ? in.lanes_request : pick_lpa(in.N, in.P, M, in.n_simds);
  r.n_blocks = (in.N * r.lpa + 63) / 64;
  r.plain = in.plain_step;
  // ordered force sum: the DPP chain for every obstacle count (round 3: with the first chunk's accumulates fused and
  // interleaved with the scaling chain it also wins for short lists -- C1, nine obstacles: 121.3 -> 111.8 us; rounds 1-2
  // switched to LDS batches below 21 obstacles). PMAF_SUM=lds selects the LDS-batch kernels (pmaf_rollout_w64.hpp; tests, timing).
  r.dpp_sum = in.dpp_sum;
  r.math = in.math;
  r.tuned_real_step = in.math == pmaf::MATH_XACT && !in.force_generic;

  // ---- the one-wave kernel of the mapping ----
  // (the wave per agent's one-slot kernel keeps lanes 61-63 for the goal and the two speed limits and lane 60 for the
  // repulsive obstacle: 61-64 obstacles go to the multi-wave / two-slot kernels)
  const int slots64 = (M >= 61 && M <= 64) ? 2 : (M + 63) / 64;
  const int slots_grp = (M + r.lpa - 1) / r.lpa;
  if (r.lpa == 64 && slots64 <= 4 && !in.force_generic) {
    r.family = WAVE_PER_AGENT;
    r.slots = slots64;
  } else if (!in.force_generic && (r.lpa == 32 || r.lpa == 16 || r.lpa == 8) && slots_grp <= 4) {
    r.family = GROUP;
    r.slots = slots_grp;
    // (policy 1, the plain fast arithmetic, exists for the w64 kernels only)
    if (in.math == pmaf::MATH_FAST) r.math = pmaf::MATH_XACT;
  } else {
    r.family = GENERIC;
    r.slots = slots_grp;
  }
  if (r.slots < 1) r.slots = 1;
  r.tiles = r.family == GENERIC ? 0 : r.slots <= 1 ? 1 : r.slots == 2 ? 2 : 4;   // (three slots run the four-slot kernels)
  // the kernels that read the closest-other table: the wave-per-agent kernels with several obstacle slots per lane, and
  // what replaces them on the same handles (the multi-wave kernel; an external kernel is the product kernel's own code)
  r.closest_table = r.family == WAVE_PER_AGENT && r.slots >= 2;

  // ---- its dynamic LDS ----
  // obstacle table + known flags, then (w64 kernels) the per-step list of circular-field terms: 64 * TILES entries of
  // 4 doubles -- w64: (64 * TILES + 8 padding + 64 scratch) entries; groups: 64 * TILES + one zero entry per group (<= 8).
  // TILES of the kernel routed above, never below 2 (pmaf_list_area_doubles): with the four-slot size a one-wave block of
  // 129 obstacles asks for 18.5 KB + the kernel's 2.1 KB of static LDS (exp's table) -- over the 20 KB that let eight
  // blocks share a CU, and 2048+ agents x 128 obstacles ran at 7/8 occupancy with a second round of blocks (+45 %: the
  // request had been sized by a second copy of the ladder above that had drifted from it).
  // The generic kernel uses none of the list area and has always asked for the four-slot size; the figure is what
  // pmaf_get_launch_config reports, so it stays.
  {
    const size_t n_obs = (size_t)M + 1;
    size_t off = 7 * n_obs + (n_obs + 1) / 2;
    off += off & 1;
    r.lds_rollout = sizeof(double) * (off + (size_t)pmaf::pmaf_list_area_doubles(r.tiles ? r.tiles : 4) + 8 * 4);
  }

  // ---- W waves per agent with <= 61 obstacles each (pmaf_k_mw.hip) instead of 2 / 4 obstacle slots per lane of ONE wave:
  // the per-obstacle part of the step runs on W SIMDs at once. Every policy but the compiler-IEEE one. Only while the
  // launch leaves every BLOCK a CU of its own (N P <= CUs of the device) -- beyond that the multi-slot kernels' single
  // wave per agent wins back.
  // PMAF_MW=0 / 2 / 3 / 4: off / that many waves (tests, timing); PMAF_MW_PER: obstacles per wave (default: even split).
  r.waves = 1;
  r.per = M;
  if (r.family == WAVE_PER_AGENT && in.math != pmaf::MATH_IEEE && M >= 61 && M <= 4 * 64 && in.mw != 0 && !in.mw_refused) {
    // as few waves as hold the obstacles at 64 per wave (every wave more costs ~0.24 us per step: profiles/r4_ab_mw.txt);
    // at <= 61 per wave lanes 61..63 stay free for the tail's riders and the sweep's norms ride along (pmaf_k_mw.hip)
    int waves = (M + 63) / 64;
    if (waves < 2) waves = 2;
    if (in.mw >= waves && in.mw <= 4) waves = in.mw;
    // ONE block per CU (pmaf_k_mw.hip's launcher enforces it through the LDS request). Rounds 4's rule let two two-wave
    // blocks share a CU (N P <= 2 CUs); measured in round 5 (profiles/r5_mw_rule_sweep.txt, 300 steps, kernel us per launch):
    //   128 obstacles: 256 agents split 536 / one-wave 578, 288 ... 512 agents split 710 ... 716 / one-wave 601
    //   100 obstacles: 256 agents 492 / 550, 384 ... 512 agents 649 ... 652 / 574;   64 obstacles: 445 / 515, 616 ... 621 / 540
    // -- as soon as ONE CU holds two blocks (their four waves contend for the CU's LDS pipe at the per-step hand-off) the
    // launch is 18 % slower than the two-slot one-wave kernel, so the split kernel is kept to launches with a CU per block.
    if (agents <= (long)(in.n_simds / 4)) {
      int per = (M + waves - 1) / waves;
      if (in.mw_per >= per && in.mw_per <= 64) per = in.mw_per;
      r.family = MULTI_WAVE;
      r.waves = waves;
      r.per = per;
      r.mw_lds_kb = in.mw_lds_kb;
    }
  }

  // ---- two waves of the wave-per-agent kernel on one SIMD (1 025 ... 2 048 agents in the handle) trade issue priority in
  // slices of the wall clock so that both finish together (pmaf_k_w64.hip, SLICE; pmaf_get_priority_slices).
  // tools/slicesweep.py, profiles/r6_slice_sweep.txt, kernel us per launch without -> with (slices of 2^9 ticks = 5.1 us,
  // the younger wave 5 of 8):
  //   32 obstacles: 1 280 agents 347 -> 326, 1 536: 359 -> 334, 2 048: 381 -> 364;  9 x 2 048: 376 -> 362;  60 x 2 048: 383 -> 370;
  //   BASELINE C5, two scenes in the handle (its per-GPU load at 4 GPUs): 386 -> 372.  Settings 2^8 ... 2^10 x 4 ... 6 of 8: within 2 %.
  // The arithmetic and its order are the same instructions: bit-identical results (tests/test_parity_gpu.py runs these shapes).
  // Offered for more one-slot waves than SIMDs and at most two per SIMD, in the kernel variants that exist with the loop
  // (DPP sum, PLAIN step, strict or contracted arithmetic), and on none of the routes that bypass k_rollout_w64.
  r.sliced = in.w64_slice && r.family == WAVE_PER_AGENT && !in.external && r.slots == 1 && in.dpp_sum && in.plain_step &&
             (in.math == pmaf::MATH_XACT || in.math == pmaf::MATH_FMA) && agents > in.n_simds && agents <= 2L * in.n_simds;

  // ---- measurement tooling (tools/slackprof): the launch of the route so far with a kernel out of an external code
  // object -- the product kernel's own assembly with delay instructions inserted -- on the wave-per-agent grid with
  // lds_rollout; the other figures stay what the handle reported without it
  if (in.external) r.family = EXTERNAL;

  // ---- the repulsive track: k_rollout_w64_track is the one-slot wave-per-agent kernel (both ordered sums, PLAIN and
  // general step) of the default arithmetic policy, without the priority-slicing loop
  r.carries_track = r.family == WAVE_PER_AGENT && r.slots == 1 && r.tiles == 1 && in.math == pmaf::MATH_XACT && !r.sliced;
  // ---- the obstacle tracks: k_rollout_w64_ftrack is the same kernel with the tracked field obstacles
  r.carries_field_tracks = r.carries_track;
  return r;
}

}  // namespace pmaf_route
