// pmaf_host.cpp -- host side of libpmaf_hip.so: the C-ABI of include/pmaf.h (handle, buffers, streams, the tick
// protocol, the repulsive track and the obstacle tracks, the stepping API, getters, profiling) over the kernels of pmaf_k_*.hip (launch
// interface: pmaf_types.hpp). The path audit and the selections: pmaf_host_audit.cpp; the winner-record exchange and
// the peer mailboxes: pmaf_host_exchange.cpp; checkpointing: pmaf_host_state.cpp (shared: pmaf_host_impl.hpp).
// Plain C++ against the HIP runtime API; there is no CPU fallback in this library.
#include <functional>

#include "pmaf_host_impl.hpp"

static thread_local std::string g_err;
void pmaf_set_last_error(const std::string &msg) { g_err = msg; }  // every host unit and pmaf_shard.cpp report through this channel

void pmaf_host::aos_to_soa(const double *aos, double *soa, int P, int n_obs) {
  for (int p = 0; p < P; p++)
    for (int i = 0; i < n_obs; i++)
      for (int c = 0; c < 7; c++) soa[((size_t)p * 7 + c) * n_obs + i] = aos[((size_t)p * n_obs + i) * 7 + c];
}

// smallest z >= 0 with sqrt(z) > c, i.e. (sqrt(z) > c) == (z >= sq_gt(c)) for all z >= 0.
// std::sqrt is correctly rounded on the host and bit-identical to the device's
// (tests/test_parity_gpu.py::test_device_arithmetic_is_ieee_exact).
static double sq_gt(double c) {
  double z = c * c;
  while (z > 0.0 && std::sqrt(z) > c) z = std::nextafter(z, 0.0);
  while (!(std::sqrt(z) > c)) z = std::nextafter(z, INFINITY);
  return z;
}
// smallest z >= 0 with sqrt(z) >= c, i.e. (sqrt(z) < c) == (z < sq_ge(c))
static double sq_ge(double c) {
  double z = c * c;
  while (z > 0.0 && std::sqrt(z) >= c) z = std::nextafter(z, 0.0);
  while (!(std::sqrt(z) >= c)) z = std::nextafter(z, INFINITY);
  return z;
}

// Boundary of the repulsive obstacle's range test (repelForce, B/src/cf_agent.cpp:168-171):
// smallest z >= 0 for which  max(sqrt(z) - R, 1e-5) < shell  is false; the predicate is
// monotone in z, so  (max(sqrt(z) - R, 1e-5) < shell) == (z < boundary).
static double repel_boundary(double R, double shell) {
  auto in_range = [&](double z) { double d = std::sqrt(z) - R; d = (d < 1e-5) ? 1e-5 : d; return d < shell; };
  if (!in_range(0.0)) return 0.0;
  double lo = 0.0, hi = 1.0;
  while (in_range(hi)) { hi *= 4.0; if (!(hi < 1e300)) return INFINITY; }
  // bisection on the ordered bit patterns of non-negative doubles
  uint64_t a, b;
  std::memcpy(&a, &lo, 8); std::memcpy(&b, &hi, 8);
  while (b - a > 1) {
    uint64_t m = a + (b - a) / 2;
    double z; std::memcpy(&z, &m, 8);
    if (in_range(z)) a = m; else b = m;
  }
  double z; std::memcpy(&z, &b, 8);
  return z;
}

// The handle's route from its inputs (pmaf_route.hpp). Called where an input changes and nowhere else: pmaf_create,
// refresh_plain_step, pmaf_debug_external_rollout, and the multi-wave launcher's refusal (dispatch_rollout) -- never per launch.
static void reroute(pmaf_planner *h) { h->route = pmaf_route::route(h->route_in); }

// Which step the wave-per-agent kernels run (pmaf_k_w64.hip, PLAIN): the one without attractorForce's `k_attr != 0`
// test and the division by the mass is only valid when every agent's k_attr is non-zero and the agents have unit mass.
// Decided where the gains / the mass enter the handle: pmaf_create and pmaf_load_state (k_attr == NULL: read them back
// from the device).
void pmaf_host::refresh_plain_step(pmaf_planner *h, const double *k_attr) {
  const size_t PN = (size_t)h->D.P * h->D.N;
  std::vector<double> tmp;
  if (!k_attr) {
    tmp.resize(PN);
    h->download(tmp.data(), h->D.k_attr, PN);
    k_attr = tmp.data();
  }
  bool plain = (h->D.C.mass == 1.0);
  for (size_t i = 0; i < PN && plain; i++) plain = (k_attr[i] != 0.0);
  const char *ps = getenv("PMAF_PLAIN_STEP");   // "0": always the general step (tests, timing)
  if (ps && ps[0] == '0') plain = false;
  h->route_in.plain_step = plain;
  reroute(h);
}

// fold finished rollout event pairs (oldest first) into the stats; all=true
// requires the stream to be idle
static void drain_events(pmaf_planner *h, bool all) {
  size_t done = 0;
  for (; done < h->ev_inflight.size(); done++) {
    auto &pr = h->ev_inflight[done];
    if (!all && hipEventQuery(pr.second) != hipSuccess) break;
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, pr.first, pr.second));
    h->rollout_ms += ms;
    h->last_rollout_ms = ms;
    h->timed_launches++;
    h->ev_free.push_back(pr);
  }
  h->ev_inflight.erase(h->ev_inflight.begin(), h->ev_inflight.begin() + (long)done);
}

// The launch the handle's route names; only forwards the route's fields.
static bool dispatch_rollout(pmaf_planner *h, hipEvent_t e0, hipEvent_t e1) {
  const pmaf_route::Route &r = h->route;
  switch (r.family) {
    case pmaf_route::EXTERNAL: {
      // (measurement tooling, tools/slackprof; events as marker packets around it)
      void *args[] = {(void *)&h->D, (void *)&h->cp};
      if (e0) HIP_CHECK(hipEventRecord(e0, h->stream));
      HIP_CHECK(hipModuleLaunchKernel(h->ext_fn, (unsigned)h->D.N, (unsigned)h->D.P, 1, 64, 1, 1, (unsigned)r.lds_rollout,
                                      h->stream, args, nullptr));
      if (e1) HIP_CHECK(hipEventRecord(e1, h->stream));
      return true;
    }
    case pmaf_route::MULTI_WAVE:
      if (pmaf_k_launch_mw(h->D, h->cp, r.waves, r.per, r.math, r.plain, r.mw_lds_kb, h->stream, e0, e1)) return true;
      // (the split kernel refused the launch -- its 72 / 96 KB LDS opt-in failed on this device, or a bad PMAF_MW_LDS_KB:
      // the one-wave kernels serve every such population, bit for bit the same; pmaf_get_waves_per_agent reports 1 from now on)
      (void)hipGetLastError();
      h->route_in.mw_refused = true;
      reroute(h);
      return dispatch_rollout(h, e0, e1);
    case pmaf_route::WAVE_PER_AGENT:
      if (h->ftrk.on()) {   // (launch_rollout has checked Route::carries_field_tracks)
        const pmaf_planner::FieldTrack &f = h->ftrk;
        const TrackArgs T = h->trk.on() ? TrackArgs{h->trk.d_pts.get(), h->trk.d_len.get(), h->trk.stride}
                                        : TrackArgs{f.d_no_pts.get(), f.d_no_len.get(), 1};
        const FTrackArgs F{f.d_pts.get(), f.d_len.get(), f.d_first.get(), f.stride};
        return pmaf_k_launch_w64_ftrack(h->D, h->cp, T, F, r.dpp_sum, r.plain, r.lds_rollout, h->stream, e0, e1);
      }
      if (h->trk.on()) {   // (launch_rollout has checked Route::carries_track)
        const TrackArgs T{h->trk.d_pts.get(), h->trk.d_len.get(), h->trk.stride};
        return pmaf_k_launch_w64_track(h->D, h->cp, T, r.dpp_sum, r.plain, r.lds_rollout, h->stream, e0, e1);
      }
      return pmaf_k_launch_w64(h->D, h->cp, r.tiles, r.math, r.dpp_sum, r.plain, r.lds_rollout, h->stream, e0, e1, r.sliced);
    case pmaf_route::GROUP:
      return pmaf_k_launch_grp(h->D, h->cp, r.lpa, r.tiles, r.math, r.n_blocks, r.lds_rollout, h->stream, e0, e1);
    case pmaf_route::GENERIC:
      break;
  }
  return pmaf_k_launch_generic(h->D, h->cp, r.lpa, r.n_blocks, r.lds_rollout, h->stream, e0, e1);
}

// A track is never silently ignored: the launch the route names must have the variant that follows it.
enum TrackKind { REPULSIVE_TRACK, FIELD_TRACKS };
static void require_track_route(const pmaf_planner *h, const pmaf_route::Route &r, const char *who, TrackKind kind = REPULSIVE_TRACK) {
  if (kind == FIELD_TRACKS ? r.carries_field_tracks : r.carries_track) return;
  fail(PMAF_ERR_STATE, std::string(who) + (kind == FIELD_TRACKS ? ": the obstacle tracks need" : ": the repulsive track needs") + " the one-slot wave-per-agent kernel of the default arithmetic "
       "policy (<= 60 field obstacles, one wave per SIMD at most); this handle's route is the " + pmaf_route::family_name(r.family) +
       " kernel" + (r.family == pmaf_route::WAVE_PER_AGENT ? (r.sliced ? " with the priority-slicing loop" : r.slots > 1 ?
       " with several obstacle slots per lane" : " of another arithmetic policy") : ""));
}

// (Re)build the device buffer from the host's copy of the upload: stride = the longest of the upload's max_len and --
// coupled -- the path capacity. Stream order; the caller has drained the stream where a rollout may still read it.
static void upload_tracks(pmaf_planner *h) {
  pmaf_planner::Track &t = h->trk;
  const int P = h->D.P;
  int need = std::max(1, t.uploaded ? t.up_max : 0);
  if (t.coupled) need = std::max(need, h->D.cap);
  t.d_len.reserve(sizeof(int32_t) * P);
  t.d_src.reserve(sizeof(int32_t) * P);
  const bool grew = t.d_pts.reserve(sizeof(double) * (size_t)P * need * 3);   // (grows exactly when need > stride)
  if (grew) t.stride = need;
  // An upload between pmaf_reset_agents and pmaf_start of a coupled handle: the coupled populations' tracks were taken in
  // front of the reset, the paths they came from are cut, and the launch will not take them again -- they stay, and only
  // the other populations' parts are rewritten (coupled: stride >= cap >= up_max, the buffer did not grow; the coupling
  // itself is unchanged, pmaf_couple_tracks drops `captured`)
  if (t.coupled && t.captured && !grew) {
    std::vector<double> one((size_t)t.stride * 3);
    for (int p = 0; p < P; p++) {
      if (t.src[p] >= 0) continue;
      const int32_t n = t.uploaded ? t.up_len[p] : 0;
      std::fill(one.begin(), one.end(), 0.0);
      if (n > 0) std::memcpy(one.data(), t.up.data() + (size_t)p * t.up_max * 3, sizeof(double) * 3 * (size_t)n);
      h->upload(t.d_pts.get() + (size_t)p * t.stride * 3, one.data(), one.size());
      h->upload(t.d_len.get() + p, &n, 1);
    }
    return;
  }
  std::vector<double> pts((size_t)P * t.stride * 3, 0.0);
  std::vector<int32_t> len(P, 0), src(P, -1);
  for (int p = 0; p < P; p++) {
    if (t.uploaded) {
      len[p] = t.up_len[p];
      std::memcpy(pts.data() + (size_t)p * t.stride * 3, t.up.data() + (size_t)p * t.up_max * 3, sizeof(double) * 3 * (size_t)len[p]);
    }
    if (t.coupled && t.src[p] >= 0) { src[p] = t.src[p]; len[p] = 0; }   // (until k_track_from_best has run)
  }
  h->upload(t.d_pts.get(), pts.data(), pts.size());
  h->upload(t.d_len.get(), len.data(), len.size());
  h->upload(t.d_src.get(), src.data(), src.size());
}

// the coupled populations' tracks <- the selected paths as they lie in the scored buffer right now (stream order)
static void capture_coupled_tracks(pmaf_planner *h) {
  const CoupleArgs A{h->trk.d_src.get(), h->D.paths, h->trk.d_pts.get(), h->trk.d_len.get(), h->trk.stride, h->trk.shift};
  pmaf_k_launch_track_from_best(h->D, A, h->stream);
  HIP_CHECK(hipGetLastError());
}

// the obstacle tracks' device-side source (pmaf_fcouple.hpp): what both of its kernels take
static FCoupleArgs fcouple_args(pmaf_planner *h) {
  const pmaf_planner::FieldTrack &f = h->ftrk;
  return FCoupleArgs{f.d_src.get(), f.d_scale.get(), f.d_anchor.get(), f.d_is_src.get(), h->D.paths, f.d_sel_pts.get(),
                     f.d_sel_n.get(), f.d_pts.get(), f.d_len.get(), f.d_first.get(), f.stride, f.shift};
}

// the source populations' selected paths -> the staging buffer, as they lie in the scored buffer right now (stream order)
static void take_field_sources(pmaf_planner *h) {
  pmaf_k_launch_fcouple_take(h->D, fcouple_args(h), h->stream);
  HIP_CHECK(hipGetLastError());
}

static void launch_rollout(pmaf_planner *h) {
  if (h->ftrk.on()) require_track_route(h, h->route, "rollout launch", FIELD_TRACKS);
  if (h->ftrk.coupled) {
    // the take at k_track_from_best's moment (below); the composition here, where obs_start is what the rollout reads
    if (!h->ftrk.captured) take_field_sources(h);
    h->ftrk.captured = false;
    pmaf_k_launch_fcouple_compose(h->D, fcouple_args(h), h->stream);
    HIP_CHECK(hipGetLastError());
  }
  if (h->trk.on()) {
    require_track_route(h, h->route, "rollout launch");   // (pmaf_start / pmaf_tick have checked already)
    // before this rollout overwrites the paths -- unless a reset in front of it already has, and took them first
    if (h->trk.coupled && !h->trk.captured) capture_coupled_tracks(h);
    h->trk.captured = false;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->profiling && (h->prof_phase++ % h->prof_every) == 0) {
    drain_events(h, false);
    if (h->ev_free.empty()) {
      hipEvent_t a, b;
      HIP_CHECK(hipEventCreate(&a));
      HIP_CHECK(hipEventCreate(&b));
      h->ev_free.emplace_back(a, b);
    }
    e0 = h->ev_free.back().first;
    e1 = h->ev_free.back().second;
    h->ev_free.pop_back();
    h->ev_inflight.emplace_back(e0, e1);   // both events ride on the rollout kernel's own dispatch (no marker packets)
  }
  // with a communicator attached the rollout writes the OTHER path buffer: the exchange of the selection just made
  // may still be packing the path it scored (the getters follow D.paths)
  if (h->x.c) h->D.paths = (h->D.paths == h->x.paths_a) ? h->x.paths_b : h->x.paths_a;
  const bool ok = dispatch_rollout(h, e0, e1);
  if (!ok) fail(PMAF_ERR_INVALID, "no rollout kernel for this lanes_per_agent / obstacle count in this build");
  HIP_CHECK(hipGetLastError());
  h->launches++;
  h->paths_gen++;
  h->scores_valid = true;
  h->cp_valid = true;
  h->rollout_pending = false;
}

void pmaf_host::sync(pmaf_planner *h) {
  HIP_CHECK(hipStreamSynchronize(h->stream));
  // an exchange in flight still reads the scored path buffer until its pack kernel is through
  for (auto &sl : h->x.slot)
    if (sl.pack_pending) { HIP_CHECK(hipEventSynchronize(sl.ev_pack)); sl.pack_pending = false; }
  if (!h->ev_inflight.empty()) drain_events(h, true);
}

static void set_cost_params(pmaf_planner *h, const double *cost_gains, const double *ws) {
  CostParams n{};
  n.k_goal_dist = cost_gains[0];
  n.k_path_len = cost_gains[1];
  n.k_safe_dist = cost_gains[2];
  n.k_workspace = cost_gains[3];
  for (int i = 0; i < 6; i++) n.ws[i] = ws[i];
  bool same_ws = h->cp_valid && n.k_workspace == h->cp.k_workspace && std::memcmp(n.ws, h->cp.ws, sizeof(n.ws)) == 0;
  h->cp = n;
  if (!same_ws) h->scores_valid = false;
  h->cp_valid = true;
}

static void ensure_scores(pmaf_planner *h) {
  if (h->scores_valid) return;
  pmaf_k_launch_score(h->D, h->cp, h->stream);
  HIP_CHECK(hipGetLastError());
  h->scores_valid = true;
}

// The caller's obstacle list (pmaf_tick, pmaf_move_real, pmaf_reset_agents): converted into the mapped pinned buffer
// k_manager reads directly. One buffer is enough: each of these calls returns only after the manager kernel that read it
// has published its result.
static const double *stage_live_obstacles_zero_copy(pmaf_planner *h, const double *obstacles) {
  if (!obstacles) return nullptr;
  const size_t n = (size_t)h->D.P * h->D.n_obs * 7;
  // the same list as the one already resident in D.obs_live (bit for bit): nothing to hand over
  // (not while peer mailboxes are connected: a coupled population's trailing row of D.obs_live is the peer's set-point then,
  // not the caller's)
  if (!h->peer.on && h->live_resident.size() == n && std::memcmp(h->live_resident.data(), obstacles, sizeof(double) * n) == 0) return nullptr;
  check_range(obstacles, n, "obstacles");
  h->note_live_obstacles(obstacles);
  h->live_resident.assign(obstacles, obstacles + n);
  aos_to_soa(obstacles, h->zc.host(), h->D.P, h->D.n_obs);
  return h->zc.dev();
}

// Staging marks the caller's list as resident BEFORE a manager kernel has read it. Whatever fails between the staging and
// that kernel's published result (an upload that throws, a launch error, a mailbox time-out): the list may not have reached
// D.obs_live, so it must not count as resident -- a retry with the same list has to hand it over again. Armed on
// construction; the caller disarms it once the mailbox result of the launch that carried the list is in.
struct ResidentGuard {
  pmaf_planner *h; bool armed = true;
  ~ResidentGuard() { if (armed) { h->live_resident.clear(); h->last_live.clear(); h->closest_dirty = true; } }
};

// a pending closed-loop position into D.real_pos the slow way (stream sync + copy), for the consumers of D.real_pos
// that are not manager launches (winner-record packing, the state blob)
void pmaf_host::flush_real_position(pmaf_planner *h) {
  if (!h->real_pos_pending) return;
  sync(h);
  h->upload(h->D.real_pos, h->real_pos_h.data(), (size_t)h->D.P * 3);
  h->real_pos_pending = false;
}

static void launch_manager(pmaf_planner *h, const ManagerArgs &A0, hipEvent_t done = nullptr) {
  ManagerArgs A = A0;
  const bool hand_over_position = h->real_pos_pending;
  if (hand_over_position) {
    if (h->D.P <= PMAF_RP_INLINE) {   // by value in the kernel arguments (no PCIe read in front of the real step)
      A.real_pos_inline = 1;
      std::memcpy(A.real_pos_val, h->rp.host(), sizeof(double) * 3 * (size_t)h->D.P);
    } else {
      A.real_pos_src = h->rp.dev();
    }
  }
  if (A.do_reset) h->paths_gen++;
  if (A.do_reset && h->route.closest_table) { A.compute_closest = h->closest_dirty ? 1 : 0; h->closest_dirty = false; }
  A.tuned_real_step = h->route.tuned_real_step ? 1 : 0;
  pmaf_k_launch_manager(h->D, h->cp, A, h->lds_manager, h->stream, done);
  HIP_CHECK(hipGetLastError());
  if (hand_over_position) h->real_pos_pending = false;   // (only once the launch that reads it is in the stream)
}

// copy the mailbox into the host-side real-agent state (call after the
// k_manager launch has completed)
static void refresh_real_cache(pmaf_planner *h) {
  for (int p = 0; p < h->D.P; p++) {
    const double *o = h->mbox.host() + p * PMAF_MBOX;
    for (int c = 0; c < 3; c++) {
      h->real_pos_h[p * 3 + c] = o[1 + c];
      h->real_vel_h[p * 3 + c] = o[4 + c];
      h->real_force_h[p * 3 + c] = o[8 + c];
    }
  }
}

// Spin until k_manager has published sequence number `seq` for every
// population. The stream is queried now and then so that a failed or finished
// launch cannot leave the host spinning.
// Bounded in wall-clock time (round 4): a hung or wedged GPU must not hang a 100 Hz control loop at 100 % CPU -- after
// PMAF_TICK_TIMEOUT_S (default 5 s) the call fails with PMAF_ERR_DEVICE (the clock is only read every 2^14 spins / on
// every poll of the blocking variant).
static void wait_mailbox(pmaf_planner *h, double seq, const char *who = "pmaf_tick") {
  bounded_wait(
      SeqWords{h->mbox.host() + 11, h->D.P, PMAF_MBOX, seq}, [&] { return hipStreamQuery(h->stream); },
      [&] {
        if (!h->blocking_wait) return spin_pause();
        // PMAF_FLAG_BLOCKING_WAIT: give the core away between polls (batch drivers that issue ticks back to back
        // would otherwise spin for the rest of the previous rollout); costs up to one sleep quantum of latency
        std::this_thread::sleep_for(std::chrono::microseconds(20));
        return 0x400u;
      },
      1u << 14, h->tick_timeout_s,
      [&] {
        // the two launches of this tick are still queued or running: they will read the zero-copy buffers and write
        // the mailbox later, so the handle takes no further tick until the stream has been drained (pmaf_stop)
        h->tick_abandoned = true;
        char msg[384];
        snprintf(msg, sizeof msg, "%s: no result from the manager kernel within the time limit (PMAF_TICK_TIMEOUT_S = %g s): "
                 "device hung, the previous rollout still running%s; call pmaf_stop() before the next tick", who, h->tick_timeout_s,
                 h->peer.on ? ", or a coupled peer's header outstanding (the in-kernel wait is bounded by PMAF_PEER_TIMEOUT_S)" : "");
        fail(PMAF_ERR_DEVICE, msg);
      },
      who, ": manager kernel finished without publishing its result");
}

static void append_real_path(pmaf_planner *h) {
  for (int p = 0; p < h->D.P; p++) {
    const double *o = h->mbox.host() + p * PMAF_MBOX;
    h->real_path[p].insert(h->real_path[p].end(), {o[1], o[2], o[3]});
  }
}

// a call that ran into the time limit left its kernels queued: they still read the staging buffers and write the mailbox
void pmaf_host::require_drained(pmaf_planner *h, const char *who) {
  if (h->tick_abandoned)
    fail(PMAF_ERR_STATE, std::string(who) + ": a previous call ran into its time limit with its kernels still queued; drain the "
                         "stream with pmaf_stop() (or recreate the handle) first");
}

// the stepping API's and the audits' obstacle list: checked, converted, uploaded (stream order, synchronised)
const double *pmaf_host::upload_plan_obstacles(pmaf_planner *h, const double *obstacles) {
  const size_t n = (size_t)h->D.P * 7 * h->D.n_obs;
  check_range(obstacles, (size_t)h->D.P * h->D.n_obs * 7, "obstacles");
  if (!h->d_plan_obs) {
    h->d_plan_obs = h->dalloc_untracked<double>(n);
    h->d_plan_out = h->dalloc_untracked<double>((size_t)h->D.P * h->D.N);
    h->d_plan_calls = h->dalloc_untracked<int32_t>((size_t)h->D.P);
  }
  std::vector<double> soa(n);
  aos_to_soa(obstacles, soa.data(), h->D.P, h->D.n_obs);
  h->upload(h->d_plan_obs, soa.data(), n);
  return h->d_plan_obs;
}

extern "C" {

const char *pmaf_last_error(void) { return g_err.c_str(); }
int pmaf_abi_version(void) { return PMAF_ABI_VERSION; }
int pmaf_eval_order(void) {
#ifdef PMAF_DOT_RIGHT_ASSOC
  return PMAF_EVAL_ORDER_DOT_RIGHT;
#else
  return PMAF_EVAL_ORDER_DOT_LEFT;
#endif
}

int pmaf_create(const pmaf_params *prm, pmaf_planner **out) {
  pmaf_planner *h = nullptr;
  int rc = guarded([&] {
    REQUIRE(prm && out, "pmaf_create: NULL argument");
    REQUIRE(prm->abi_version == PMAF_ABI_VERSION, "pmaf_create: ABI version mismatch");
    REQUIRE(prm->n_populations >= 1 && prm->n_agents >= 1, "pmaf_create: need n_populations >= 1 and n_agents >= 1");
    REQUIRE(prm->n_obstacles >= 1, "pmaf_create: obstacle list must hold at least the trailing repulsive obstacle");
    REQUIRE(prm->max_prediction_steps >= 1, "pmaf_create: max_prediction_steps must be >= 1");
    REQUIRE(prm->goal && prm->obstacles && prm->k_attr && prm->k_circ && prm->k_repel && prm->k_damp,
            "pmaf_create: goal, obstacles and gain arrays are required");
    {
      const size_t P_ = (size_t)prm->n_populations, N_ = (size_t)prm->n_agents, O_ = (size_t)prm->n_obstacles;
      check_range(prm->goal, P_ * 3, "pmaf_create: goal");
      if (prm->init_pos) check_range(prm->init_pos, P_ * 3, "pmaf_create: init_pos");
      check_range(prm->obstacles, P_ * O_ * 7, "pmaf_create: obstacles");
      check_range(prm->k_attr, P_ * N_, "pmaf_create: k_attr"); check_range(prm->k_circ, P_ * N_, "pmaf_create: k_circ");
      check_range(prm->k_repel, P_ * N_, "pmaf_create: k_repel"); check_range(prm->k_damp, P_ * N_, "pmaf_create: k_damp");
      if (prm->random_vecs) check_range(prm->random_vecs, P_ * N_ * O_ * 3, "pmaf_create: random_vecs");
      const double sc[6] = {prm->dt, prm->velocity_max, prm->approach_dist, prm->detect_shell_rad, prm->agent_mass, prm->radius};
      check_range(sc, 6, "pmaf_create: scalar parameter");
    }
    int lp = prm->lanes_per_agent;
    REQUIRE(lp == 0 || (lp >= 1 && lp <= 64 && (lp & (lp - 1)) == 0), "pmaf_create: lanes_per_agent must be 0 or a power of two <= 64");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) fail(PMAF_ERR_DEVICE, "pmaf_create: no HIP device available (this library has no CPU fallback)");
    h = new pmaf_planner();
    if (prm->device >= 0) h->device = prm->device; else HIP_CHECK(hipGetDevice(&h->device));
    REQUIRE(h->device < ndev, "pmaf_create: device ordinal out of range");
    h->use_device();
    HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&h->ev_mgr, hipEventDisableTiming));
    const int P = prm->n_populations, N = prm->n_agents, n_obs = prm->n_obstacles, cap = prm->max_prediction_steps;
    const int M = n_obs - 1;
    DevView &D = h->D;
    D.P = P; D.N = N; D.n_obs = n_obs; D.cap = cap;
    D.C.dt = prm->dt; D.C.vel_max = prm->velocity_max; D.C.approach = prm->approach_dist;
    D.C.shell = prm->detect_shell_rad; D.C.mass = prm->agent_mass; D.C.rad = prm->radius;
    D.C.zf_gt = sq_gt(1e-5); D.C.zacc_gt = sq_gt(13.0); D.C.zinit_lt = sq_ge(0.2);
    D.C.zvhalf_lt = sq_ge(0.5 * prm->velocity_max);
    D.C.zv09_lt = sq_ge(prm->velocity_max - 0.1 * prm->velocity_max);
    pmaf_route::Input &ri = h->route_in;
    ri.N = N; ri.P = P; ri.M = M; ri.lanes_request = lp;
    ri.math = (prm->flags & PMAF_FLAG_CONTRACTED) ? MATH_FMA : (prm->flags & PMAF_FLAG_FAST_MATH) ? MATH_FAST
              : (prm->flags & PMAF_FLAG_IEEE_SEQUENCES) ? MATH_IEEE : MATH_XACT;
    h->blocking_wait = (prm->flags & PMAF_FLAG_BLOCKING_WAIT) != 0;
    {
      int cus = 0;
      HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
      D.n_simds = 4 * (cus > 0 ? cus : 256);
    }
    ri.n_simds = D.n_simds;
    // the route's switches in the environment (tests, timing experiments; what each does: pmaf_route.hpp)
    { const char *fg = getenv("PMAF_FORCE_GENERIC"); ri.force_generic = fg && fg[0] == '1'; }
    { const char *e = getenv("PMAF_W64_SLICE"); ri.w64_slice = e ? (e[0] == '1') : true; }
    { const char *ds = getenv("PMAF_SUM"); ri.dpp_sum = (ds && ds[0]) ? (ds[0] == 'd') : true; }  // "dpp" / "lds"
    { const char *e = getenv("PMAF_MW"); ri.mw = (e && e[0]) ? atoi(e) : -1; }
    { const char *e = getenv("PMAF_MW_PER"); ri.mw_per = e ? atoi(e) : 0; }
    { const char *e = getenv("PMAF_MW_LDS_KB"); ri.mw_lds_kb = e ? atoi(e) : 0; }
    reroute(h);   // (plain_step still false: refresh_plain_step below, once the gains are in)
    // the priority-slicing loop's settings (PMAF_W64_SLICE_LOG2, PMAF_W64_SLICE_YOUNGER: timing experiments)
    { const char *e = getenv("PMAF_W64_SLICE_LOG2"); D.prio_slice_log2 = std::min(20, std::max(4, e ? atoi(e) : 9)); }       // (a shift count on the device)
    { const char *e = getenv("PMAF_W64_SLICE_YOUNGER"); D.prio_younger_of_8 = std::min(7, std::max(1, e ? atoi(e) : 5)); }
    { const char *to = getenv("PMAF_EXCHANGE_TIMEOUT_S"); if (to && atof(to) > 0.0) h->exchange_timeout_s = atof(to); }
    { const char *to = getenv("PMAF_TICK_TIMEOUT_S"); if (to && atof(to) > 0.0) h->tick_timeout_s = atof(to); }
    REQUIRE((M + h->route.lpa - 1) / h->route.lpa <= 64, "pmaf_create: too many obstacles for this lanes_per_agent (need M <= 64*lanes_per_agent)");
    // table | known flags | costs | the tuned real step's list (64 * 4 + 8 + 64 entries of 4 doubles)
    // (+ 2: the wave-minimum cell of circ_and_scale_w64 behind the list)
    h->lds_manager = sizeof(double) * (7 * (size_t)n_obs + ((size_t)n_obs + 1) / 2 + (size_t)N + 1 + (size_t)pmaf_list_area_doubles(4) + 2);
    REQUIRE(h->route.lds_rollout <= 160 * 1024, "pmaf_create: obstacle table does not fit in LDS");
    REQUIRE(h->lds_manager <= 160 * 1024,
            "pmaf_create: n_agents + obstacle table exceed the manager kernel's LDS budget (160 KB: 8 B per agent, 60 B per obstacle)");
    // dynamic LDS beyond the 64 KB default needs the per-function opt-in
    HIP_CHECK(pmaf_k_set_lds_limits(h->lds_manager, h->route.lds_rollout));

    size_t PN = (size_t)P * N;
    double *goal = h->dalloc<double>(P * 3);
    D.goal = goal;
    D.agent_init_pos = h->dalloc<double>(P * 3);
    D.start_pos = h->dalloc<double>(P * 3);
    D.start_vel = h->dalloc<double>(P * 3);
    D.obs_start = h->dalloc<double>((size_t)P * 7 * n_obs);
    D.known_start = h->dalloc<int32_t>((size_t)P * n_obs);
    D.obs_live = h->dalloc<double>((size_t)P * 7 * n_obs);
    D.closest_idx = h->dalloc<int32_t>((size_t)P * n_obs);   // (zero-filled; closest_ok = 0: no table yet)
    D.closest_ok = h->dalloc<int32_t>((size_t)P);
    double *ka = h->dalloc<double>(PN), *kc = h->dalloc<double>(PN), *kr = h->dalloc<double>(PN), *kd = h->dalloc<double>(PN);
    D.k_attr = ka; D.k_circ = kc; D.k_repel = kr; D.k_damp = kd;
    int32_t *types = h->dalloc<int32_t>(N);
    D.types = types;
    D.rot = h->dalloc<double>(PN * 3 * n_obs);
    double *rnd = h->dalloc<double>(PN * 3 * n_obs);
    D.rnd = rnd;
    D.paths = h->dalloc<double>(PN * (size_t)cap * 3);
    D.n_points = h->dalloc<int32_t>(PN);
    D.agent_vel = h->dalloc<double>(PN * 3);
    D.min_obs = h->dalloc<double>(PN);
    D.cost_ws = h->dalloc<double>(PN);
    D.path_len = h->dalloc<double>(PN);
    D.goal_dist = h->dalloc<double>(PN);
    D.reached = h->dalloc<int32_t>(PN);
    D.known_out = h->dalloc<int32_t>(PN * n_obs);
    D.costs = h->dalloc<double>(PN);
    D.real_pos = h->dalloc<double>(P * 3);
    D.real_vel = h->dalloc<double>(P * 3);
    D.real_force = h->dalloc<double>(P * 3);
    D.real_init_pos = h->dalloc<double>(P * 3);
    D.real_known = h->dalloc<int32_t>((size_t)P * n_obs);
    D.real_rot = h->dalloc<double>((size_t)P * 3 * n_obs);
    D.has_best = h->dalloc<int32_t>(P);
    D.best_id = h->dalloc<int32_t>(P);
    D.best_type = h->dalloc<int32_t>(P);
    D.best_rnd = h->dalloc<double>((size_t)P * 3 * n_obs);
    D.best_idx = h->dalloc<int32_t>(P);
    D.step_counter = h->dalloc<unsigned long long>(1);
    D.pred_ticks = h->dalloc<unsigned long long>(PN);
    double *zsent = h->dalloc<double>(P);
    D.zsent_lt = zsent;
    h->d_reset_in = h->dalloc<double>(P * 6);
    h->d_agent_id = h->dalloc<int32_t>(P);
    h->mbox.alloc(sizeof(double) * P * PMAF_MBOX);
    h->zc.alloc(sizeof(double) * (size_t)P * 7 * n_obs);
    h->rp.alloc(sizeof(double) * (size_t)P * 3);

    // ---- initial state = freshly constructed agents (cf_agent.h:69-97) ----
    std::vector<double> init(P * 3, 0.0);
    if (prm->init_pos) init.assign(prm->init_pos, prm->init_pos + P * 3);
    h->goal_h.assign(prm->goal, prm->goal + P * 3);
    h->upload(goal, prm->goal, P * 3);
    // CfAgent::init_pos_ member starts at zero (cf_agent.h:78), positions at CfManager::init_pos_
    h->upload(D.start_pos, init.data(), P * 3);
    h->upload(D.real_pos, init.data(), P * 3);
    std::vector<double> v0(P * 3, 0.0);
    for (int p = 0; p < P; p++) v0[p * 3] = 0.01;  // vel_{0.01, 0, 0}, cf_agent.h:76
    h->upload(D.start_vel, v0.data(), P * 3);
    h->upload(D.real_vel, v0.data(), P * 3);
    std::vector<double> soa((size_t)P * 7 * n_obs);
    aos_to_soa(prm->obstacles, soa.data(), P, n_obs);
    {
      std::vector<double> zs(P);
      for (int p = 0; p < P; p++)
        zs[p] = repel_boundary(prm->radius + prm->obstacles[((size_t)p * n_obs + (n_obs - 1)) * 7 + 6], prm->detect_shell_rad);
      h->upload(zsent, zs.data(), P);
    }
    h->upload(D.obs_start, soa.data(), soa.size());
    h->upload(D.obs_live, soa.data(), soa.size());
    h->live_resident.assign(prm->obstacles, prm->obstacles + (size_t)P * n_obs * 7);
    h->upload(ka, prm->k_attr, PN); h->upload(kc, prm->k_circ, PN);
    refresh_plain_step(h, prm->k_attr);
    h->upload(kr, prm->k_repel, PN); h->upload(kd, prm->k_damp, PN);
    std::vector<int32_t> ty(N);
    static const int layout[5] = {PMAF_HAD_HEURISTIC, PMAF_GOAL_HEURISTIC, PMAF_OBSTACLE_HEURISTIC,
                                  PMAF_GOAL_OBSTACLE_HEURISTIC, PMAF_VEL_HEURISTIC};
    for (int i = 0; i < N; i++) {
      ty[i] = prm->agent_types ? prm->agent_types[i] : (i < 5 ? layout[i] : PMAF_RANDOM_AGENT);
      REQUIRE(ty[i] >= PMAF_GOAL_HEURISTIC && ty[i] <= PMAF_HAD_HEURISTIC, "pmaf_create: agent type must be one of the six heuristics");
    }
    h->upload(types, ty.data(), N);
    // rotation vectors start at (0,0,1), cf_agent.h:92-96; component-major [3][n_obs]
    {
      std::vector<double> rot(PN * 3 * n_obs, 0.0);
      for (size_t pa = 0; pa < PN; pa++)
        for (int i = 0; i < n_obs; i++) rot[(pa * 3 + 2) * n_obs + i] = 1.0;
      h->upload(D.rot, rot.data(), rot.size());
      std::vector<double> rr((size_t)P * 3 * n_obs, 0.0);
      for (int p = 0; p < P; p++)
        for (int i = 0; i < n_obs; i++) rr[((size_t)p * 3 + 2) * n_obs + i] = 1.0;
      h->upload(D.real_rot, rr.data(), rr.size());
    }
    if (prm->random_vecs) {
      std::vector<double> r(PN * 3 * n_obs);
      for (size_t pa = 0; pa < PN; pa++)
        for (int i = 0; i < n_obs; i++)
          for (int c = 0; c < 3; c++) r[(pa * 3 + c) * n_obs + i] = prm->random_vecs[(pa * n_obs + i) * 3 + c];
      h->upload(rnd, r.data(), r.size());
    }
    // 1-point paths at init_pos, min_obs = shell
    {
      std::vector<double> paths(PN * (size_t)cap * 3, 0.0);
      std::vector<int32_t> np(PN, 1);
      std::vector<double> mo(PN, prm->detect_shell_rad), av(PN * 3, 0.0);
      for (size_t pa = 0; pa < PN; pa++) {
        int p = (int)(pa / N);
        for (int c = 0; c < 3; c++) paths[pa * cap * 3 + c] = init[p * 3 + c];
        av[pa * 3] = 0.01;
      }
      h->upload(D.paths, paths.data(), paths.size());
      h->upload(D.n_points, np.data(), np.size());
      h->upload(D.min_obs, mo.data(), mo.size());
      h->upload(D.agent_vel, av.data(), av.size());
    }
    h->real_pos_h = init;
    h->real_vel_h = v0;
    h->real_force_h.assign(P * 3, 0.0);
    h->real_path.assign(P, {});
    for (int p = 0; p < P; p++) h->real_path[p].insert(h->real_path[p].end(), {init[p * 3], init[p * 3 + 1], init[p * 3 + 2]});
    h->rollout_pending = true;
    sync(h);
    *out = h;
  });
  if (rc != PMAF_OK && h) { pmaf_destroy(h); }
  return rc;
}

int pmaf_destroy(pmaf_planner *h) {
  if (!h) return PMAF_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  detach_comm(h);
  peer_disconnect(h);
  if (h->ext_mod) (void)hipModuleUnload(h->ext_mod);
  for (void *p : h->allocs) (void)hipFree(p);
  for (void *p : h->scratch) (void)hipFree(p);
  for (auto &e : h->ev_free) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (auto &e : h->ev_inflight) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (h->ev_mgr) (void)hipEventDestroy(h->ev_mgr);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;   // the scratch and the pinned memory go with their owners (pmaf_host_impl.hpp)
  return PMAF_OK;
}

int pmaf_set_initial_position(pmaf_planner *h, const double *pos) {
  return guarded([&] {
    REQUIRE(h && pos, "pmaf_set_initial_position: NULL argument");
    check_range(pos, (size_t)h->D.P * 3, "pmaf_set_initial_position");
    h->use_device();
    sync(h);
    DevView &D = h->D;
    const int P = D.P;
    h->upload(D.agent_init_pos, pos, P * 3);
    h->upload(D.real_init_pos, pos, P * 3);
    h->upload(D.real_pos, pos, P * 3);
    h->real_pos_pending = false;   // (a closed-loop position handed over before this call is superseded)
    h->upload(D.start_pos, pos, P * 3);
    // CfAgent::setPosition = clear + push_back for every predicted agent
    h->paths_gen++;
    h->trk.captured = false;   // (the paths start over: nothing taken from the old ones is followed)
    h->ftrk.captured = false;
    pmaf_k_launch_restart_paths(D, D.start_pos, h->stream);
    HIP_CHECK(hipGetLastError());
    h->real_pos_h.assign(pos, pos + P * 3);
    for (int p = 0; p < P; p++)  // RealCfAgent::setPosition = push_back
      h->real_path[p].insert(h->real_path[p].end(), {pos[p * 3], pos[p * 3 + 1], pos[p * 3 + 2]});
    sync(h);
    h->scores_valid = false;
    h->rollout_pending = true;
    h->stepped = false;
  });
}

int pmaf_set_real_position(pmaf_planner *h, const double *pos) {
  return guarded([&] {
    REQUIRE(h && pos, "pmaf_set_real_position: NULL argument");
    check_range(pos, (size_t)h->D.P * 3, "pmaf_set_real_position");
    if (h->tick_abandoned)   // (its manager kernel may not have read the staging buffer yet)
      fail(PMAF_ERR_STATE, "pmaf_set_real_position: the previous tick ran into its time limit; call pmaf_stop() first");
    // RealCfAgent::setPosition = push_back (B/src/cf_agent.cpp:44-46): the measured position becomes the real agent's
    // latest one. Handed to the next manager launch through mapped pinned memory -- no wait for the running rollout,
    // no copy command (the node calls this in front of every tick when open_loop is false,
    // B/src/panda_bimanual_control.cpp:333-335)
    std::memcpy(h->rp.host(), pos, sizeof(double) * (size_t)h->D.P * 3);
    h->real_pos_pending = true;
    h->real_pos_h.assign(pos, pos + h->D.P * 3);
    for (int p = 0; p < h->D.P; p++)
      h->real_path[p].insert(h->real_path[p].end(), {pos[p * 3], pos[p * 3 + 1], pos[p * 3 + 2]});
  });
}

int pmaf_start(pmaf_planner *h) {
  return guarded([&] {
    REQUIRE(h, "pmaf_start: NULL handle");
    h->use_device();
    if (h->stepped)
      fail(PMAF_ERR_STATE, "pmaf_start: the agents were moved / set by the stepping API (pmaf_move_agent(s), pmaf_set_agent_*); "
                           "call pmaf_reset_agents or pmaf_set_initial_position first (rollouts start from the population's reset state)");
    // a finished rollout that was not reset has nothing left to predict
    // (guard B/src/cf_agent.cpp:310-311 is already false)
    if (!h->rollout_pending) return;
    if (h->trk.on()) require_track_route(h, h->route, "pmaf_start");
    if (h->ftrk.on()) require_track_route(h, h->route, "pmaf_start", FIELD_TRACKS);
    if (!h->cp_valid) {  // no evaluate yet: score with neutral workspace terms, rescored on evaluate
      h->cp = CostParams{};
      h->cp.ws[0] = h->cp.ws[2] = h->cp.ws[4] = INFINITY;
      h->cp.ws[1] = h->cp.ws[3] = h->cp.ws[5] = -INFINITY;
    }
    bool had_cp = h->cp_valid;
    launch_rollout(h);
    h->cp_valid = had_cp;
    if (!had_cp) h->scores_valid = false;
  });
}

// ---- repulsive track ----
// attach / detach: the route's `tracked` input follows, and an attach the routed launch cannot carry is refused here
// (check_tracked: the refusal alone, for a call that may still refuse for another reason before it attaches)
static void check_tracked(const pmaf_planner *h, const char *who, TrackKind kind) {
  bool pmaf_route::Input::*flag = (kind == FIELD_TRACKS) ? &pmaf_route::Input::field_tracked : &pmaf_route::Input::tracked;
  pmaf_route::Input in = h->route_in;
  in.*flag = true;
  require_track_route(h, pmaf_route::route(in), who, kind);
}
static void set_tracked(pmaf_planner *h, bool want, const char *who, TrackKind kind = REPULSIVE_TRACK) {
  bool pmaf_route::Input::*flag = (kind == FIELD_TRACKS) ? &pmaf_route::Input::field_tracked : &pmaf_route::Input::tracked;
  if (want) check_tracked(h, who, kind);
  h->route_in.*flag = want;
  reroute(h);
}

int pmaf_set_repulsive_track(pmaf_planner *h, const double *track, const int32_t *len, int32_t max_len) {
  return guarded([&] {
    REQUIRE(h, "pmaf_set_repulsive_track: NULL handle");
    h->use_device();
    require_drained(h, "pmaf_set_repulsive_track");
    pmaf_planner::Track &t = h->trk;
    const int P = h->D.P;
    bool any = false;
    if (track && len) {
      REQUIRE(max_len >= 1, "pmaf_set_repulsive_track: max_len must be >= 1");
      for (int p = 0; p < P; p++) {
        REQUIRE(len[p] >= 0 && len[p] <= max_len, "pmaf_set_repulsive_track: need 0 <= len <= max_len");
        check_range(track + (size_t)p * max_len * 3, (size_t)len[p] * 3, "pmaf_set_repulsive_track: track");
        any = any || len[p] > 0;
      }
    }
    if (any) set_tracked(h, true, "pmaf_set_repulsive_track");
    sync(h);   // a running rollout still reads the buffer
    t.uploaded = any;
    if (any) {
      // (points past the path capacity are never read: the rollout has at most cap - 1 steps)
      t.up_max = std::min((int)max_len, h->D.cap);
      t.up_len.assign(P, 0);
      t.up.assign((size_t)P * t.up_max * 3, 0.0);
      for (int p = 0; p < P; p++) {
        t.up_len[p] = std::min((int)len[p], t.up_max);
        std::memcpy(t.up.data() + (size_t)p * t.up_max * 3, track + (size_t)p * max_len * 3, sizeof(double) * 3 * (size_t)t.up_len[p]);
      }
    } else {
      t.up.clear(); t.up_len.clear(); t.up_max = 0;
    }
    if (t.on()) upload_tracks(h);
    else set_tracked(h, false, "pmaf_set_repulsive_track");
  });
}

int pmaf_couple_tracks(pmaf_planner *h, const int32_t *src_pop, int32_t shift) {
  return guarded([&] {
    REQUIRE(h, "pmaf_couple_tracks: NULL handle");
    h->use_device();
    require_drained(h, "pmaf_couple_tracks");
    pmaf_planner::Track &t = h->trk;
    const int P = h->D.P;
    bool any = false;
    if (src_pop) {
      REQUIRE(shift >= 0, "pmaf_couple_tracks: shift must be >= 0");
      for (int p = 0; p < P; p++) {
        REQUIRE(src_pop[p] < P && src_pop[p] != p, "pmaf_couple_tracks: src_pop must be another population of this handle (or -1)");
        any = any || src_pop[p] >= 0;
      }
    }
    if (any) set_tracked(h, true, "pmaf_couple_tracks");
    sync(h);
    t.coupled = any;
    t.captured = false;
    if (any) {
      t.src.assign(P, -1);
      for (int p = 0; p < P; p++) t.src[p] = src_pop[p] >= 0 ? src_pop[p] : -1;
      t.shift = shift;
    } else {
      t.src.clear(); t.shift = 0;
    }
    if (t.on()) upload_tracks(h);
    else set_tracked(h, false, "pmaf_couple_tracks");
  });
}

int pmaf_get_repulsive_track(pmaf_planner *h, double *track, int32_t *len, int32_t max_len) {
  return guarded([&] {
    REQUIRE(h && len, "pmaf_get_repulsive_track: NULL argument");
    h->use_device();
    sync(h);
    const pmaf_planner::Track &t = h->trk;
    const int P = h->D.P;
    for (int p = 0; p < P; p++) len[p] = 0;
    if (!t.on() || !t.d_pts.get()) return;
    h->download(len, t.d_len.get(), P);
    if (!track) return;
    std::vector<double> pts((size_t)P * t.stride * 3);
    h->download(pts.data(), t.d_pts.get(), pts.size());
    for (int p = 0; p < P; p++) {
      REQUIRE(len[p] <= max_len, "pmaf_get_repulsive_track: max_len is shorter than a track");
      std::memcpy(track + (size_t)p * max_len * 3, pts.data() + (size_t)p * t.stride * 3, sizeof(double) * 3 * (size_t)len[p]);
    }
  });
}

// ---- obstacle tracks ----
// The small buffers every launch of k_rollout_w64_ftrack is handed: the lengths and offsets, and the one-point,
// zero-length repulsive track of a handle without one. Allocated by the first attach or coupling.
static void reserve_ftrack_aux(pmaf_planner *h) {
  pmaf_planner::FieldTrack &f = h->ftrk;
  const int P = h->D.P;
  if (f.d_len.reserve(sizeof(int32_t) * P)) HIP_CHECK(hipMemsetAsync(f.d_len.get(), 0, sizeof(int32_t) * P, h->stream));
  if (f.d_first.reserve(sizeof(int32_t) * P)) HIP_CHECK(hipMemsetAsync(f.d_first.get(), 0, sizeof(int32_t) * P, h->stream));
  if (f.d_no_pts.reserve(sizeof(double) * (size_t)P * 3)) HIP_CHECK(hipMemsetAsync(f.d_no_pts.get(), 0, sizeof(double) * (size_t)P * 3, h->stream));
  if (f.d_no_len.reserve(sizeof(int32_t) * P)) HIP_CHECK(hipMemsetAsync(f.d_no_len.get(), 0, sizeof(int32_t) * P, h->stream));
}

// Grow the points' buffer to `need` points per population and KEEP what it holds (the host has no copy of the points): a
// coupled handle's buffer is shared between the composed populations and the uploaded ones, and either side may outgrow
// it while the other's points are still followed. The caller has drained the stream. The points stay on the device: the
// larger buffer is zeroed and filled beside the old one, one copy per population to its new stride, and then takes its
// place (a failed allocation leaves the old buffer and its stride as they were).
static void grow_ftrack_keeping(pmaf_planner *h, int need) {
  pmaf_planner::FieldTrack &f = h->ftrk;
  const int P = h->D.P, old = f.stride;
  if (f.d_pts.get() && need <= old) return;
  DeviceBuf<double> grown;
  const size_t bytes = sizeof(double) * (size_t)P * need * PMAF_FTRACK_POINT;
  grown.reserve(bytes);
  HIP_CHECK(hipMemsetAsync(grown.get(), 0, bytes, h->stream));
  if (f.d_pts.get() && old > 0)
    for (int p = 0; p < P; p++)
      HIP_CHECK(hipMemcpyAsync(grown.get() + (size_t)p * need * PMAF_FTRACK_POINT, f.d_pts.get() + (size_t)p * old * PMAF_FTRACK_POINT,
                               sizeof(double) * (size_t)old * PMAF_FTRACK_POINT, hipMemcpyDeviceToDevice, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  f.d_pts.swap(grown);
  f.stride = need;
}

// The caller's lengths, as every setter of uploaded obstacle tracks holds them: inside [0, max_len], 0 for a coupled
// population; per_pop(p) is the setter's own look at population p's values, at the place of the loop where the host
// call has it. Returns whether any population has points.
static bool ftrack_lens(pmaf_planner *h, const int32_t *len, int32_t max_len, const std::string &who,
                        const std::function<void(int)> &per_pop) {
  const pmaf_planner::FieldTrack &f = h->ftrk;
  bool any = false;
  REQUIRE(max_len >= 1, who + ": max_len must be >= 1");
  for (int p = 0; p < h->D.P; p++) {
    REQUIRE(len[p] >= 0 && len[p] <= max_len, who + ": need 0 <= len <= max_len");
    REQUIRE(len[p] == 0 || !f.is_coupled(p), who + ": the population's tracks come from pmaf_couple_obstacle_tracks (len must be 0)");
    per_pop(p);
    any = any || len[p] > 0;
  }
  return any;
}

// What a setter books once its points are accepted: attached, the lengths (len == NULL: none), every offset 0 ...
static void book_ftrack_lens(pmaf_planner *h, const int32_t *len) {
  pmaf_planner::FieldTrack &f = h->ftrk;
  const int P = h->D.P;
  f.attached = len != nullptr;
  f.first.assign(P, 0);
  f.len.assign(P, 0);
  for (int p = 0; p < P && len; p++) f.len[p] = len[p];
}
// ... and their device copies: the coupled populations' len and first are the device's (k_fcouple_compose), the others'
// are replaced one population at a time
static void upload_ftrack_lens(pmaf_planner *h) {
  pmaf_planner::FieldTrack &f = h->ftrk;
  const int P = h->D.P;
  // (one wait for all of them: the host copies are the handle's own and outlive it)
  if (!f.coupled) {
    HIP_CHECK(hipMemcpyAsync(f.d_len.get(), f.len.data(), sizeof(int32_t) * P, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(f.d_first.get(), f.first.data(), sizeof(int32_t) * P, hipMemcpyHostToDevice, h->stream));
  } else {
    for (int p = 0; p < P; p++) {
      if (f.is_coupled(p)) continue;
      HIP_CHECK(hipMemcpyAsync(f.d_len.get() + p, &f.len[p], sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
      HIP_CHECK(hipMemcpyAsync(f.d_first.get() + p, &f.first[p], sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    }
  }
  HIP_CHECK(hipStreamSynchronize(h->stream));
}
// every len == 0 (or no tracks given): the uploaded tracks go, a coupling stays. The caller has drained the stream.
static void detach_uploaded_ftracks(pmaf_planner *h, const char *who) {
  pmaf_planner::FieldTrack &f = h->ftrk;
  book_ftrack_lens(h, nullptr);
  if (!f.coupled) set_tracked(h, false, who, FIELD_TRACKS);
  if (f.d_len.get()) upload_ftrack_lens(h);   // (the getter reads them)
}

int pmaf_set_obstacle_tracks(pmaf_planner *h, const double *tracks, const int32_t *len, int32_t max_len) {
  return guarded([&] {
    REQUIRE(h, "pmaf_set_obstacle_tracks: NULL handle");
    h->use_device();
    require_drained(h, "pmaf_set_obstacle_tracks");
    pmaf_planner::FieldTrack &f = h->ftrk;
    const int P = h->D.P, M = h->D.n_obs - 1;
    bool any = false;
    if (tracks && len)
      any = ftrack_lens(h, len, max_len, "pmaf_set_obstacle_tracks", [&](int p) {
        check_range(tracks + (size_t)p * max_len * M * 6, (size_t)len[p] * M * 6, "pmaf_set_obstacle_tracks: tracks");
      });
    if (any) set_tracked(h, true, "pmaf_set_obstacle_tracks", FIELD_TRACKS);
    sync(h);   // a running rollout still reads the buffers
    if (!any) {
      detach_uploaded_ftracks(h, "pmaf_set_obstacle_tracks");
      return;
    }
    book_ftrack_lens(h, len);
    if (f.coupled) {
      // the coupled populations' points, len and first are the device's (k_fcouple_compose): the others' are replaced one
      // population at a time, and a buffer that has to grow keeps what it holds
      grow_ftrack_keeping(h, (int)max_len);
      std::vector<double> pts((size_t)f.stride * PMAF_FTRACK_POINT);
      for (int p = 0; p < P; p++) {
        if (f.is_coupled(p)) continue;
        std::fill(pts.begin(), pts.end(), 0.0);
        for (int k = 0; k < f.len[p]; k++) {
          const double *src = tracks + ((size_t)p * max_len + k) * M * 6;
          double *dst = pts.data() + (size_t)k * PMAF_FTRACK_POINT;
          for (int i = 0; i < M; i++)
            for (int c = 0; c < 6; c++) dst[c * PMAF_FTRACK_LANES + i] = src[i * 6 + c];
        }
        h->upload(f.d_pts.get() + (size_t)p * f.stride * PMAF_FTRACK_POINT, pts.data(), pts.size());
      }
      upload_ftrack_lens(h);
      return;
    }
    // the device layout (pmaf_ftrack.hpp): [P][stride][6][64], transposed here; a population's points lie at its own
    // stride, so a shorter upload into a grown buffer leaves the tail of the longer one behind it, never read
    if (f.d_pts.reserve(sizeof(double) * (size_t)P * std::max(f.stride, (int)max_len) * PMAF_FTRACK_POINT)) f.stride = std::max(f.stride, (int)max_len);
    reserve_ftrack_aux(h);
    std::vector<double> pts((size_t)P * f.stride * PMAF_FTRACK_POINT, 0.0);
    for (int p = 0; p < P; p++)
      for (int k = 0; k < f.len[p]; k++) {
        const double *src = tracks + ((size_t)p * max_len + k) * M * 6;
        double *dst = pts.data() + ((size_t)p * f.stride + k) * PMAF_FTRACK_POINT;
        for (int i = 0; i < M; i++)
          for (int c = 0; c < 6; c++) dst[c * PMAF_FTRACK_LANES + i] = src[i * 6 + c];
      }
    h->upload(f.d_pts.get(), pts.data(), pts.size());
    upload_ftrack_lens(h);
  });
}

// The memory a device source names, as the handle's device reads it -- decided before anything is enqueued: a kernel
// that reads what the device cannot map faults, and a shared machine pays for that. `bytes`: from d_tracks to the end
// of the last element that will be read.
static const void *readable_source(pmaf_planner *h, const void *d_tracks, size_t bytes, const std::string &who) {
  hipPointerAttribute_t a{};
  const hipError_t e = hipPointerGetAttributes(&a, d_tracks);
  if (e != hipSuccess) {   // (runtimes that do not know the pointer at all say so with an error)
    (void)hipGetLastError();
    fail(PMAF_ERR_INVALID, who + ": d_tracks is not memory the runtime knows (pageable host memory? copy it with pmaf_set_obstacle_tracks)");
  }
  const void *src = d_tracks;
  switch (a.type) {
    case hipMemoryTypeDevice:
      if (a.device != h->device) {
        // Readable only where the CALLER has enabled peer access from the handle's device (the current one). The runtime
        // answers that question in one way: enabling it again says "already enabled". Where it was not, the call has
        // just enabled it: that is taken back at once, and the source is refused -- the process's device state is the
        // caller's to change.
        int can = 0;
        HIP_CHECK(hipDeviceCanAccessPeer(&can, h->device, a.device));
        hipError_t pe = can ? hipDeviceEnablePeerAccess(a.device, 0) : hipErrorInvalidDevice;
        if (pe == hipSuccess) (void)hipDeviceDisablePeerAccess(a.device);
        (void)hipGetLastError();
        if (pe != hipErrorPeerAccessAlreadyEnabled)
          fail(PMAF_ERR_INVALID, who + ": d_tracks lies on device " + std::to_string(a.device) + ", to which the handle's device " +
               std::to_string(h->device) + " has no peer access enabled (hipDeviceEnablePeerAccess is the caller's to call)");
      }
      break;
    case hipMemoryTypeHost:      // pinned or registered: the device reads it through its alias
      if (a.devicePointer) src = a.devicePointer;
      break;
    case hipMemoryTypeManaged:
      break;
    default:                     // unregistered (pageable) host memory, arrays
      fail(PMAF_ERR_INVALID, who + ": d_tracks is not memory the handle's device can read (pageable host memory? copy it with pmaf_set_obstacle_tracks)");
  }
  // where the runtime can tell: the last element read lies inside the allocation
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(src)) == hipSuccess && base && size) {
    const char *lo = static_cast<const char *>(base), *at = static_cast<const char *>(src);
    if (at < lo || bytes > size || (size_t)(at - lo) > size - bytes)
      fail(PMAF_ERR_INVALID, who + ": the tracks to be read (" + std::to_string(bytes) + " bytes) run past the end of d_tracks' allocation");
  } else {
    (void)hipGetLastError();
  }
  return src;
}

int pmaf_set_obstacle_tracks_device(pmaf_planner *h, const void *d_tracks, const int32_t *len, int32_t max_len,
                                    int32_t components, int32_t dtype, void *producer_stream) {
  return guarded([&] {
    const char *who = "pmaf_set_obstacle_tracks_device";
    REQUIRE(h, "pmaf_set_obstacle_tracks_device: NULL handle");
    h->use_device();
    require_drained(h, who);
    REQUIRE(d_tracks && len, "pmaf_set_obstacle_tracks_device: NULL argument (detaching is pmaf_set_obstacle_tracks(h, NULL, NULL, 0))");
    REQUIRE(components == 6 || components == 3, "pmaf_set_obstacle_tracks_device: components must be 6 or 3");
    REQUIRE(dtype == PMAF_TRACK_F64 || dtype == PMAF_TRACK_F32, "pmaf_set_obstacle_tracks_device: unknown dtype (PMAF_TRACK_F64, PMAF_TRACK_F32)");
    const size_t esz = dtype == PMAF_TRACK_F64 ? sizeof(double) : sizeof(float);
    REQUIRE(((uintptr_t)d_tracks & (esz - 1)) == 0, "pmaf_set_obstacle_tracks_device: d_tracks is not aligned to its element type");
    pmaf_planner::FieldTrack &f = h->ftrk;
    const int P = h->D.P, M = h->D.n_obs - 1;
    const bool any = ftrack_lens(h, len, max_len, who, [](int) {});
    if (!any) {
      sync(h);
      detach_uploaded_ftracks(h, who);
      return;
    }
    size_t bytes = 0;   // ... to the end of the last population's last point
    for (int p = 0; p < P; p++)
      if (len[p] > 0) bytes = ((size_t)p * max_len + (size_t)len[p]) * M * components * esz;
    const void *src = readable_source(h, d_tracks, bytes, who);
    check_tracked(h, who, FIELD_TRACKS);
    sync(h);   // a running rollout still reads the buffers
    // nothing a refusal would have to undo: buffers that exist, a buffer that grew with what it held
    reserve_ftrack_aux(h);
    f.d_in_len.reserve(sizeof(int32_t) * P);
    f.d_verdict.reserve(sizeof(unsigned long long));
    grow_ftrack_keeping(h, std::max(f.stride, (int)max_len));
    std::vector<int32_t> in((size_t)P);
    for (int p = 0; p < P; p++) in[p] = f.is_coupled(p) ? -1 : len[p];
    // (no wait of its own: `in` lives until the verdict's copy has been waited for, behind both kernels)
    HIP_CHECK(hipMemcpyAsync(f.d_in_len.get(), in.data(), sizeof(int32_t) * in.size(), hipMemcpyHostToDevice, h->stream));
    if (producer_stream) {   // everything enqueued there up to now, without a word to the host
      hipEvent_t ev = nullptr;
      HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(producer_stream));
      if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, ev, 0);
      (void)hipEventDestroy(ev);   // (released once the record has completed)
      HIP_CHECK(e);
    }
    HIP_CHECK(hipMemsetAsync(f.d_verdict.get(), 0xFF, sizeof(unsigned long long), h->stream));
    const FtIngestArgs A{src, f.d_in_len.get(), f.d_pts.get(), f.d_verdict.get(), (int)max_len, f.stride, M, h->D.C.dt};
    pmaf_k_launch_ftingest(A, P, components, dtype, h->stream);
    HIP_CHECK(hipGetLastError());
    unsigned long long key = 0;
    h->download(&key, f.d_verdict.get(), 1);   // (waits for both kernels: the source may be overwritten from here on)
    if (key != PMAF_FTINGEST_CLEAN) {
      // the key's order: [P][max_len][M][6]
      const int c = (int)(key % 6), i = (int)(key / 6 % (unsigned long long)M);
      const unsigned long long pk = key / 6 / (unsigned long long)M;
      fail(PMAF_ERR_INVALID, std::string(who) + ": tracks: population " + std::to_string(pk / (unsigned long long)max_len) + ", point " +
           std::to_string(pk % (unsigned long long)max_len) + ", obstacle " + std::to_string(i) + ", component " + std::to_string(c) +
           (components == 3 && c >= 3 ? " (the velocity derived from this point and the next)" : "") +
           ": value outside the supported numeric range (finite, 0 or 2^-100 <= |x| <= 2^100)");
    }
    set_tracked(h, true, who, FIELD_TRACKS);
    book_ftrack_lens(h, len);
    upload_ftrack_lens(h);
  });
}

int pmaf_couple_obstacle_tracks(pmaf_planner *h, const int32_t *src_pop, const double *scale, const double *anchor, int32_t shift) {
  return guarded([&] {
    REQUIRE(h, "pmaf_couple_obstacle_tracks: NULL handle");
    h->use_device();
    require_drained(h, "pmaf_couple_obstacle_tracks");
    pmaf_planner::FieldTrack &f = h->ftrk;
    const int P = h->D.P, M = h->D.n_obs - 1, cap = h->D.cap;
    bool any = false;
    std::vector<char> pc((size_t)P, 0);
    if (src_pop) {
      REQUIRE(scale && anchor, "pmaf_couple_obstacle_tracks: scale and anchor must be given with src_pop");
      REQUIRE(shift >= 0, "pmaf_couple_obstacle_tracks: shift must be >= 0");
      for (int p = 0; p < P; p++)
        for (int i = 0; i < M; i++) {
          const int32_t q = src_pop[(size_t)p * M + i];
          REQUIRE(q >= -1 && q < P && q != p, "pmaf_couple_obstacle_tracks: src_pop must be another population of this handle (or -1)");
          if (q >= 0) pc[p] = 1;
        }
      check_range(scale, (size_t)P * M, "pmaf_couple_obstacle_tracks: scale");
      check_range(anchor, (size_t)P * M * 3, "pmaf_couple_obstacle_tracks: anchor");
      for (int p = 0; p < P; p++) {
        any = any || pc[p];
        if (pc[p] && f.attached && f.len[p] > 0)
          fail(PMAF_ERR_STATE, "pmaf_couple_obstacle_tracks: the population has uploaded obstacle tracks (detach them with pmaf_set_obstacle_tracks first)");
      }
    }
    if (any) set_tracked(h, true, "pmaf_couple_obstacle_tracks", FIELD_TRACKS);
    sync(h);   // a running rollout still reads the buffers
    // populations that stop being coupled go back to "no tracks"; the uploaded ones keep theirs
    std::vector<char> was = f.coupled ? f.pop_coupled : std::vector<char>((size_t)P, 0);
    f.captured = false;
    if (!any) {
      f.coupled = false;
      f.src.clear(); f.pop_coupled.clear(); f.shift = 0;
      const int32_t zero = 0;
      for (int p = 0; p < P; p++)
        if (was[p]) { h->upload(f.d_len.get() + p, &zero, 1); h->upload(f.d_first.get() + p, &zero, 1); }
      if (!f.attached) set_tracked(h, false, "pmaf_couple_obstacle_tracks", FIELD_TRACKS);
      return;
    }
    reserve_ftrack_aux(h);
    grow_ftrack_keeping(h, std::max(cap, 1));
    f.d_src.reserve(sizeof(int32_t) * (size_t)P * PMAF_FTRACK_LANES);
    f.d_scale.reserve(sizeof(double) * (size_t)P * PMAF_FTRACK_LANES);
    f.d_anchor.reserve(sizeof(double) * (size_t)P * 3 * PMAF_FTRACK_LANES);
    f.d_is_src.reserve(sizeof(int32_t) * P);
    f.d_sel_n.reserve(sizeof(int32_t) * P);
    f.d_sel_pts.reserve(sizeof(double) * (size_t)P * cap * 3);
    std::vector<int32_t> src((size_t)P * PMAF_FTRACK_LANES, -1), is_src((size_t)P, 0), zeros((size_t)P, 0);
    std::vector<double> sc((size_t)P * PMAF_FTRACK_LANES, 0.0), an((size_t)P * 3 * PMAF_FTRACK_LANES, 0.0);
    for (int p = 0; p < P; p++)
      for (int i = 0; i < M && i < PMAF_FTRACK_LANES; i++) {   // (the route has M <= 60)
        const int32_t q = src_pop[(size_t)p * M + i];
        src[(size_t)p * PMAF_FTRACK_LANES + i] = q;
        if (q >= 0) is_src[q] = 1;
        sc[(size_t)p * PMAF_FTRACK_LANES + i] = scale[(size_t)p * M + i];
        for (int c = 0; c < 3; c++) an[((size_t)p * 3 + c) * PMAF_FTRACK_LANES + i] = anchor[((size_t)p * M + i) * 3 + c];
      }
    f.coupled = true;
    f.src.assign(src_pop, src_pop + (size_t)P * M);
    f.pop_coupled = pc;
    f.shift = shift;
    h->upload(f.d_src.get(), src.data(), src.size());
    h->upload(f.d_scale.get(), sc.data(), sc.size());
    h->upload(f.d_anchor.get(), an.data(), an.size());
    h->upload(f.d_is_src.get(), is_src.data(), is_src.size());
    h->upload(f.d_sel_n.get(), zeros.data(), zeros.size());   // (nothing taken yet)
    HIP_CHECK(hipMemsetAsync(f.d_sel_pts.get(), 0, sizeof(double) * (size_t)P * cap * 3, h->stream));
    // L = 0 until the first composed launch, for the populations that are coupled now or were before
    const int32_t zero = 0;
    for (int p = 0; p < P; p++)
      if (pc[p] || was[p]) { h->upload(f.d_len.get() + p, &zero, 1); h->upload(f.d_first.get() + p, &zero, 1); }
  });
}

int pmaf_set_obstacle_track_offset(pmaf_planner *h, const int32_t *first) {
  return guarded([&] {
    REQUIRE(h && first, "pmaf_set_obstacle_track_offset: NULL argument");
    h->use_device();
    require_drained(h, "pmaf_set_obstacle_track_offset");
    pmaf_planner::FieldTrack &f = h->ftrk;
    const int P = h->D.P;
    for (int p = 0; p < P; p++) REQUIRE(first[p] >= 0, "pmaf_set_obstacle_track_offset: first must be >= 0");
    if (!f.on()) fail(PMAF_ERR_STATE, "pmaf_set_obstacle_track_offset: no obstacle tracks are attached (pmaf_set_obstacle_tracks)");
    for (int p = 0; p < P; p++)
      REQUIRE(first[p] == 0 || !f.is_coupled(p), "pmaf_set_obstacle_track_offset: the population's tracks come from pmaf_couple_obstacle_tracks (first must be 0)");
    f.first.assign(first, first + P);
    h->upload(f.d_first.get(), f.first.data(), (size_t)P);   // (stream order: behind a running rollout)
  });
}

int pmaf_get_obstacle_tracks(pmaf_planner *h, double *tracks, int32_t *len, int32_t *first, int32_t max_len) {
  return guarded([&] {
    REQUIRE(h && len, "pmaf_get_obstacle_tracks: NULL argument");
    h->use_device();
    sync(h);
    const pmaf_planner::FieldTrack &f = h->ftrk;
    const int P = h->D.P, M = h->D.n_obs - 1;
    for (int p = 0; p < P; p++) { len[p] = 0; if (first) first[p] = 0; }
    if (!f.on() || !f.d_pts.get()) return;
    h->download(len, f.d_len.get(), P);
    if (first) h->download(first, f.d_first.get(), P);
    if (!tracks) return;
    std::vector<double> pts((size_t)P * f.stride * PMAF_FTRACK_POINT);
    h->download(pts.data(), f.d_pts.get(), pts.size());
    for (int p = 0; p < P; p++) {
      REQUIRE(len[p] <= max_len, "pmaf_get_obstacle_tracks: max_len is shorter than a population's tracks");
      for (int k = 0; k < len[p]; k++) {
        const double *src = pts.data() + ((size_t)p * f.stride + k) * PMAF_FTRACK_POINT;
        double *dst = tracks + ((size_t)p * max_len + k) * M * 6;
        for (int i = 0; i < M; i++)
          for (int c = 0; c < 6; c++) dst[i * 6 + c] = src[c * PMAF_FTRACK_LANES + i];
      }
    }
  });
}

int pmaf_stop(pmaf_planner *h) {
  return guarded([&] {
    REQUIRE(h, "pmaf_stop: NULL handle");
    h->use_device();
    sync(h);
    h->tick_abandoned = false;   // the stream is empty: an abandoned tick's kernels are through
  });
}

int pmaf_evaluate(pmaf_planner *h, const double *cost_gains, const double *ws, int32_t *best_idx) {
  return guarded([&] {
    REQUIRE(h && cost_gains && ws, "pmaf_evaluate: NULL argument");
    h->use_device();
    require_drained(h, "pmaf_evaluate");
    set_cost_params(h, cost_gains, ws);
    ensure_scores(h);
    ManagerArgs A{};
    A.do_select = 1;
    A.out = h->mbox.dev();
    if (h->x.c) {
      A.winner_hdr = claim_exchange_slot(h).d_send;  // (its exchange of two selections ago is through)
      A.winner_stride = (int)winner_rec(h);
    }
    // (sequence numbers of the manager launches that are not ticks count down from -1; the host waits for the mailbox,
    // as pmaf_tick does, instead of for the stream: the result is on the host when the selection is published)
    A.seq = (h->call_seq -= 1.0);
    if (h->wp.host()) {   // the winner path of this selection
      A.wp_out = h->wp.dev(); A.wp_hdr = h->wph.dev();
      h->wp_seq = A.seq;
      h->wp_timed = true;
    }
    launch_manager(h, A);
    wait_mailbox(h, A.seq, "pmaf_evaluate");
    h->has_best_h = 1;
    if (h->x.c) begin_exchange(h, h->D.paths);
    if (!h->ev_inflight.empty()) drain_events(h, false);
    refresh_real_cache(h);
    if (best_idx)
      for (int p = 0; p < h->D.P; p++) best_idx[p] = (int32_t)h->mbox.host()[p * PMAF_MBOX];
  });
}

int pmaf_move_real(pmaf_planner *h, const double *obstacles, double dt, int32_t steps, const int32_t *agent_id) {
  return guarded([&] {
    REQUIRE(h && agent_id, "pmaf_move_real: NULL argument");
    REQUIRE(steps >= 0, "pmaf_move_real: steps must be >= 0");
    h->use_device();
    require_drained(h, "pmaf_move_real");
    if (h->has_best_h < 0) {   // unknown (restored / set from outside): read it back once
      sync(h);
      int32_t hb = 0;
      h->download(&hb, h->D.has_best, 1);
      h->has_best_h = hb ? 1 : 0;
    }
    if (!h->has_best_h) fail(PMAF_ERR_STATE, "pmaf_move_real: no best agent yet (call pmaf_evaluate first; the reference dereferences a null best_agent_ here)");
    for (int p = 0; p < h->D.P; p++) REQUIRE(agent_id[p] >= 0 && agent_id[p] < h->D.N, "pmaf_move_real: agent_id out of range");
    // the call's small inputs travel like pmaf_tick's: the obstacle list through the mapped pinned buffer (not at all when
    // it is the resident one), the agent indices by value in the kernel arguments (<= 4 populations), the result through
    // the mailbox -- no copy command and no stream synchronisation (round 5; the node's five calls 106 -> ~45 us)
    // steps == 0: no manager launch reads the list, so it is not staged either (staging marks it resident; a later call
    // with the same list would then hand nothing over and plan on the old obstacles). The reference's moveRealEEAgent
    // passes the list to cfPlanner inside its steps loop only (B/src/cf_manager.cpp:257-263): zero steps leave no trace.
    if (steps == 0) return;
    ResidentGuard resident_guard{h};
    const double *live = stage_live_obstacles_zero_copy(h, obstacles);
    const bool inl = h->D.P <= PMAF_RP_INLINE;
    if (!inl) h->upload(h->d_agent_id, agent_id, h->D.P);
    for (int s = 0; s < steps; s++) {
      ManagerArgs A{};
      A.do_move = 1;
      A.dt_real = dt;
      if (inl) { A.agent_id_inline = 1; for (int p = 0; p < h->D.P; p++) A.agent_id_val[p] = agent_id[p]; }
      else A.agent_id = h->d_agent_id;
      A.live_src = (s == 0) ? live : nullptr;
      A.out = h->mbox.dev();
      A.seq = (h->call_seq -= 1.0);
      launch_manager(h, A);
      wait_mailbox(h, A.seq, "pmaf_move_real");
      resident_guard.armed = false;   // the first launch has read the list (later ones use D.obs_live)
      refresh_real_cache(h);
      append_real_path(h);
    }
  });
}

int pmaf_reset_agents(pmaf_planner *h, const double *pos, const double *vel, const double *obstacles) {
  return guarded([&] {
    REQUIRE(h && pos && vel, "pmaf_reset_agents: NULL argument");
    check_range(pos, (size_t)h->D.P * 3, "pmaf_reset_agents: pos");
    check_range(vel, (size_t)h->D.P * 3, "pmaf_reset_agents: vel");
    h->use_device();
    require_drained(h, "pmaf_reset_agents");
    // an exchange in flight still reads the scored path buffer until its pack kernel is through (the reset rewrites the
    // paths' first points); everything else is ordered by the stream
    for (auto &sl : h->x.slot)
      if (sl.pack_pending) { HIP_CHECK(hipEventSynchronize(sl.ev_pack)); sl.pack_pending = false; }
    // coupled tracks: the reset below cuts every path to its first point, so the selected paths are taken here
    if (h->trk.coupled) { capture_coupled_tracks(h); h->trk.captured = true; }
    if (h->ftrk.coupled) { take_field_sources(h); h->ftrk.captured = true; }
    ResidentGuard resident_guard{h};
    const double *live = stage_live_obstacles_zero_copy(h, obstacles);
    ManagerArgs A{};
    A.do_reset = 1;
    if (h->D.P <= PMAF_RP_INLINE) {
      A.reset_in_inline = 1;
      for (int p = 0; p < h->D.P; p++)
        for (int c = 0; c < 3; c++) { A.reset_in_val[p * 6 + c] = pos[p * 3 + c]; A.reset_in_val[p * 6 + 3 + c] = vel[p * 3 + c]; }
    } else {
      std::vector<double> in(h->D.P * 6);
      for (int p = 0; p < h->D.P; p++)
        for (int c = 0; c < 3; c++) { in[p * 6 + c] = pos[p * 3 + c]; in[p * 6 + 3 + c] = vel[p * 3 + c]; }
      h->upload(h->d_reset_in, in.data(), in.size());
    }
    A.reset_in = h->d_reset_in;
    A.live_src = live;
    A.out = h->mbox.dev();
    A.seq = (h->call_seq -= 1.0);
    // The mailbox is published once the kernel has read EVERY input of this call (the pinned obstacle list, d_reset_in:
    // both are loaded in front of the publication in k_manager) -- the staging buffers are free again -- and BEFORE its
    // reset stores (obs_start, known_start, the agents' state). Invariant the host relies on for those: whatever reads
    // or overwrites them next is either a launch on h->stream (ordered behind this kernel) or a getter that calls sync().
    launch_manager(h, A);
    wait_mailbox(h, A.seq, "pmaf_reset_agents");
    resident_guard.armed = false;
    refresh_real_cache(h);
    h->scores_valid = false;
    h->rollout_pending = true;
    h->stepped = false;
  });
}

int pmaf_tick(pmaf_planner *h, const double *obstacles, double dt, const double *cost_gains, const double *ws,
              int32_t *best_idx, double *next_pos, double *next_vel) {
  return guarded([&] {
    REQUIRE(h && cost_gains && ws, "pmaf_tick: NULL argument");
    const auto t_entry = std::chrono::steady_clock::now();
    h->use_device();
    require_drained(h, "pmaf_tick");
    if (h->trk.on()) require_track_route(h, h->route, "pmaf_tick");   // (before anything is launched)
    if (h->ftrk.on()) require_track_route(h, h->route, "pmaf_tick", FIELD_TRACKS);
    // whatever fails between here and the manager kernel's result: the list handed over with this call may not have
    // reached D.obs_live, so it must not count as resident (a retry with the same list has to hand it over again)
    ResidentGuard resident_guard{h};
    set_cost_params(h, cost_gains, ws);
    ensure_scores(h);
    ManagerArgs A{};
    A.live_src = stage_live_obstacles_zero_copy(h, obstacles);
    A.do_select = 1; A.do_move = 1; A.do_reset = 1; A.reset_from_real = 1;
    A.rollout_follows = 1;
    A.dt_real = dt;
    A.out = h->mbox.dev();
    const double want_seq = (double)(++h->mailbox_seq);
    A.seq = h->dbg_withhold ? 0.0 : want_seq;   // (fault injection: pmaf_debug_withhold_mailbox)
    if (h->wp.host()) { A.wp_out = h->wp.dev(); A.wp_hdr = h->wph.dev(); h->wp_seq = A.seq; h->wp_timed = false; h->last_tick_entry = t_entry; }
    if (h->x.c) {
      // the send buffer of the exchange two ticks back (long through); the previous tick's collective is NOT waited for
      A.winner_hdr = claim_exchange_slot(h).d_send;
      A.winner_stride = (int)winner_rec(h);
    }
    if (h->peer.on) {
      A.peer = h->peer.d_view;
      A.peer_tick = (double)(++h->peer.tick);
    }
    launch_manager(h, A);
    const double *scored = h->D.paths;  // the paths this selection scored; the rollout below writes the other buffer
    h->rollout_pending = true;
    h->stepped = false;
    launch_rollout(h);
    const auto t_enq = std::chrono::steady_clock::now();
    // outputs of k_manager land in mapped pinned memory; wait for them only
    // (no event between the two launches: the host polls the sequence number -- spinning, or with
    // PMAF_FLAG_BLOCKING_WAIT sleeping between polls)
    wait_mailbox(h, want_seq);
    {
      const auto t_sp = std::chrono::steady_clock::now();
      if (h->tick_enq_us.empty()) { h->tick_enq_us.resize(pmaf_planner::TICK_RING); h->tick_sp_us.resize(pmaf_planner::TICK_RING); }
      h->tick_enq_us[h->tick_head] = std::chrono::duration<float, std::micro>(t_enq - t_entry).count();
      h->tick_sp_us[h->tick_head] = std::chrono::duration<float, std::micro>(t_sp - t_entry).count();
      h->tick_head = (h->tick_head + 1) % pmaf_planner::TICK_RING;
      if (h->tick_count < pmaf_planner::TICK_RING) h->tick_count++;
    }
    resident_guard.armed = false;   // the manager kernel has read the list and published its result
    h->has_best_h = 1;
    const int peer_late = h->peer.on ? peer_book_tick(h) : 0;
    if (h->x.c) begin_exchange(h, scored);  // pack + all-gather on the exchange stream, beside the rollout
    refresh_real_cache(h);
    append_real_path(h);
    for (int p = 0; p < h->D.P; p++) {
      const double *o = h->mbox.host() + p * PMAF_MBOX;
      if (best_idx) best_idx[p] = (int32_t)o[0];
      if (next_pos) { next_pos[p * 3] = o[1]; next_pos[p * 3 + 1] = o[2]; next_pos[p * 3 + 2] = o[3]; }
      if (next_vel) { next_vel[p * 3] = o[4]; next_vel[p * 3 + 1] = o[5]; next_vel[p * 3 + 2] = o[6]; }
    }
    if (peer_late == 1)
      fail(PMAF_ERR_DEVICE, "pmaf_tick: the header of a coupled peer population did not arrive in time (a peer rank behind "
                            "by more than PMAF_PEER_TIMEOUT_S, or gone); the trailing obstacle kept its previous value");
    if (peer_late == 2)
      fail(PMAF_ERR_STATE, "pmaf_tick: a coupled peer population had already overwritten the header this tick needs (it ran "
                           "ahead): couplings must be pairwise mutual and every rank must issue the same pmaf_tick calls "
                           "(include/pmaf.h, peer mailboxes: TOPOLOGY); the trailing obstacle kept its previous value");
    if (peer_late == 3)
      fail(PMAF_ERR_STATE, "pmaf_tick: a coupled peer population is not coupled back to this one -- couplings must be "
                           "pairwise mutual (include/pmaf.h, peer mailboxes: TOPOLOGY)");
  });
}

// ---- synchronous stepping API ----
static void plan_steps(pmaf_planner *h, const double *obstacles, double dt, int steps, const int32_t *agent_id,
                       int max_calls, int32_t *calls) {
  check_range(&dt, 1, "dt");
  h->use_device();
  sync(h);
  const DevView &D = h->D;
  std::vector<int32_t> np((size_t)D.P * D.N);
  h->download(np.data(), D.n_points, np.size());
  if (!agent_id) {  // moveAgents: every path must have room for `steps` more points
    int mx = 0;
    for (int32_t v : np) mx = v > mx ? v : mx;
    if ((long)mx + steps > (long)D.cap)
      fail(PMAF_ERR_STATE, "pmaf_move_agents: a path would outgrow max_prediction_steps (the path buffers are fixed-size)");
  }
  PlanArgs A{};
  A.obs = upload_plan_obstacles(h, obstacles);
  A.dt = dt;
  A.steps = steps;
  A.max_calls = agent_id ? max_calls : 1;
  A.until_goal = agent_id ? 1 : 0;
  if (agent_id) {
    for (int p = 0; p < D.P; p++) REQUIRE(agent_id[p] >= 0 && agent_id[p] < D.N, "pmaf_move_agent: agent_id out of range");
    h->upload(h->d_agent_id, agent_id, D.P);
    A.only = h->d_agent_id;
    A.calls_out = h->d_plan_calls;
    HIP_CHECK(hipMemsetAsync(h->d_plan_calls, 0, sizeof(int32_t) * D.P, h->stream));
  }
  h->paths_gen++;
  if (!pmaf_k_launch_plan_steps(D, A, h->route.lpa, h->route.n_blocks, h->route.lds_rollout, h->stream)) fail(PMAF_ERR_INVALID, "bad lanes_per_agent");
  HIP_CHECK(hipGetLastError());
  sync(h);
  if (agent_id && calls) h->download(calls, h->d_plan_calls, D.P);
  h->scores_valid = false;     // path costs are re-scored on demand (k_score)
  h->rollout_pending = false;
  h->stepped = true;
}

int pmaf_move_agents(pmaf_planner *h, const double *obstacles, double dt, int32_t steps) {
  return guarded([&] {
    REQUIRE(h && obstacles, "pmaf_move_agents: NULL argument");
    REQUIRE(steps >= 0, "pmaf_move_agents: steps must be >= 0");
    plan_steps(h, obstacles, dt, steps, nullptr, 1, nullptr);
  });
}

int pmaf_move_agent(pmaf_planner *h, const double *obstacles, double dt, int32_t steps, const int32_t *agent_id,
                    int32_t max_calls, int32_t *calls) {
  return guarded([&] {
    REQUIRE(h && obstacles && agent_id, "pmaf_move_agent: NULL argument");
    REQUIRE(steps >= 1 && max_calls >= 0, "pmaf_move_agent: need steps >= 1 and max_calls >= 0");
    plan_steps(h, obstacles, dt, steps, agent_id, max_calls, calls);
  });
}

static void set_agents(pmaf_planner *h, const double *pos, const double *vel) {
  const int P = h->D.P;
  check_range(pos, (size_t)P * 3, "pos");
  if (vel) check_range(vel, (size_t)P * 3, "vel");
  h->use_device();
  sync(h);
  std::vector<double> in((size_t)P * 6, 0.0);
  for (int p = 0; p < P; p++)
    for (int c = 0; c < 3; c++) { in[p * 6 + c] = pos[p * 3 + c]; if (vel) in[p * 6 + 3 + c] = vel[p * 3 + c]; }
  // d_reset_in holds [P][6]; the kernel takes two [P][3] arrays: repack
  std::vector<double> pk((size_t)P * 6);
  for (int p = 0; p < P; p++)
    for (int c = 0; c < 3; c++) { pk[p * 3 + c] = in[p * 6 + c]; pk[(size_t)P * 3 + p * 3 + c] = in[p * 6 + 3 + c]; }
  h->upload(h->d_reset_in, pk.data(), pk.size());
  h->paths_gen++;
  pmaf_k_launch_set_agents(h->D, h->d_reset_in, vel ? h->d_reset_in + (size_t)P * 3 : nullptr, h->stream);
  HIP_CHECK(hipGetLastError());
  sync(h);
  h->scores_valid = false;
  h->rollout_pending = false;
  // like after pmaf_move_agent(s): in the reference a startPrediction() here would continue with each agent's OWN
  // velocity, known flags and advanced obstacle copies (CfAgent::setPosition only clears the path,
  // B/src/cf_agent.cpp:39-42), which a rollout launched from the population's reset state cannot reproduce
  h->stepped = true;
}

int pmaf_set_agent_positions(pmaf_planner *h, const double *pos) {
  return guarded([&] {
    REQUIRE(h && pos, "pmaf_set_agent_positions: NULL argument");
    set_agents(h, pos, nullptr);
  });
}

int pmaf_set_agent_pos_and_vels(pmaf_planner *h, const double *pos, const double *vel) {
  return guarded([&] {
    REQUIRE(h && pos && vel, "pmaf_set_agent_pos_and_vels: NULL argument");
    set_agents(h, pos, vel);
  });
}

#define GETTER_PROLOGUE(name)                    \
  REQUIRE(h, name ": NULL handle");              \
  h->use_device();                               \
  sync(h);                                       \
  const DevView &D = h->D;                       \
  const size_t PN = (size_t)D.P * D.N;           \
  (void)PN;

// bring the host mirror of paths / n_points up to date (one D2H per rollout generation)
static void refresh_paths_mirror(pmaf_planner *h) {
  if (h->mirror_gen == h->paths_gen) return;
  const DevView &D = h->D;
  const size_t PN = (size_t)D.P * D.N;
  h->h_paths.reserve(sizeof(double) * PN * (size_t)D.cap * 3);
  h->h_np.reserve(sizeof(int32_t) * PN);
  HIP_CHECK(hipMemcpyAsync(h->h_np.get(), D.n_points, sizeof(int32_t) * PN, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipMemcpyAsync(h->h_paths.get(), D.paths, sizeof(double) * PN * (size_t)D.cap * 3, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  // entries past an agent's path end are stale device memory: report zeros
  for (size_t pa = 0; pa < PN; pa++)
    std::memset(h->h_paths.get() + (pa * D.cap + h->h_np.get()[pa]) * 3, 0, sizeof(double) * 3 * (size_t)(D.cap - h->h_np.get()[pa]));
  h->mirror_gen = h->paths_gen;
}

int pmaf_get_paths(pmaf_planner *h, double *paths, int32_t *n_points) {
  return guarded([&] {
    GETTER_PROLOGUE("pmaf_get_paths")
    refresh_paths_mirror(h);
    if (paths) std::memcpy(paths, h->h_paths.get(), sizeof(double) * PN * (size_t)D.cap * 3);
    if (n_points) std::memcpy(n_points, h->h_np.get(), sizeof(int32_t) * PN);
  });
}
// zero-copy view of the same mirror: *paths [P][N][cap][3] and *n_points [P][N] stay valid until the next call that
// changes the predicted paths (start / tick / reset / set_* / move_agents / load_state)
int pmaf_view_paths(pmaf_planner *h, const double **paths, const int32_t **n_points) {
  return guarded([&] {
    GETTER_PROLOGUE("pmaf_view_paths")
    refresh_paths_mirror(h);
    if (paths) *paths = h->h_paths.get();
    if (n_points) *n_points = h->h_np.get();
  });
}
int pmaf_get_costs(pmaf_planner *h, double *costs) {
  return guarded([&] { GETTER_PROLOGUE("pmaf_get_costs") REQUIRE(costs, "NULL out"); h->download(costs, D.costs, PN); });
}
int pmaf_get_path_lengths(pmaf_planner *h, double *out) {
  return guarded([&] {
    GETTER_PROLOGUE("pmaf_get_path_lengths")
    REQUIRE(out, "NULL out");
    if (!h->cp_valid) {
      h->cp = CostParams{};
      h->cp.ws[0] = h->cp.ws[2] = h->cp.ws[4] = INFINITY;
      h->cp.ws[1] = h->cp.ws[3] = h->cp.ws[5] = -INFINITY;
    }
    bool had = h->cp_valid;
    ensure_scores(h);
    if (!had) h->scores_valid = false;
    sync(h);
    h->download(out, D.path_len, PN);
  });
}
int pmaf_get_min_obs_dist(pmaf_planner *h, double *out) {
  return guarded([&] { GETTER_PROLOGUE("pmaf_get_min_obs_dist") REQUIRE(out, "NULL out"); h->download(out, D.min_obs, PN); });
}
int pmaf_get_success(pmaf_planner *h, int32_t *out) {
  return guarded([&] { GETTER_PROLOGUE("pmaf_get_success") REQUIRE(out, "NULL out"); h->download(out, D.reached, PN); });
}
int pmaf_get_agent_velocities(pmaf_planner *h, double *out) {
  return guarded([&] { GETTER_PROLOGUE("pmaf_get_agent_velocities") REQUIRE(out, "NULL out"); h->download(out, D.agent_vel, PN * 3); });
}
int pmaf_get_rotation_vectors(pmaf_planner *h, double *rot, int32_t *known) {
  return guarded([&] {
    GETTER_PROLOGUE("pmaf_get_rotation_vectors")
    const int n_obs = D.n_obs;
    if (rot) {
      std::vector<double> r(PN * 3 * n_obs);
      h->download(r.data(), D.rot, r.size());
      for (size_t pa = 0; pa < PN; pa++)
        for (int i = 0; i < n_obs; i++)
          for (int c = 0; c < 3; c++) rot[(pa * n_obs + i) * 3 + c] = r[(pa * 3 + c) * n_obs + i];
    }
    if (known) h->download(known, D.known_out, PN * n_obs);
  });
}
int pmaf_get_real_state(pmaf_planner *h, double *pos, double *vel, double *force) {
  return guarded([&] {
    // served from the host copy kept current by every call that changes the real
    // agent: no wait for the running rollout (the reference's getters are instant)
    REQUIRE(h, "pmaf_get_real_state: NULL handle");
    const size_t n = sizeof(double) * 3 * (size_t)h->D.P;
    if (pos) std::memcpy(pos, h->real_pos_h.data(), n);
    if (vel) std::memcpy(vel, h->real_vel_h.data(), n);
    if (force) std::memcpy(force, h->real_force_h.data(), n);
  });
}
int pmaf_get_real_known(pmaf_planner *h, int32_t *known, double *rot) {
  return guarded([&] {
    GETTER_PROLOGUE("pmaf_get_real_known")
    const int n_obs = D.n_obs;
    if (known) h->download(known, D.real_known, (size_t)D.P * n_obs);
    if (rot) {
      std::vector<double> r((size_t)D.P * 3 * n_obs);
      h->download(r.data(), D.real_rot, r.size());
      for (int p = 0; p < D.P; p++)
        for (int i = 0; i < n_obs; i++)
          for (int c = 0; c < 3; c++) rot[((size_t)p * n_obs + i) * 3 + c] = r[((size_t)p * 3 + c) * n_obs + i];
    }
  });
}
int pmaf_get_real_path(pmaf_planner *h, int32_t pop, double *out, int32_t max_points, int32_t *n_total) {
  return guarded([&] {
    REQUIRE(h && pop >= 0 && pop < h->D.P, "pmaf_get_real_path: bad argument");
    const std::vector<double> &rp = h->real_path[pop];
    int n = (int)(rp.size() / 3);
    if (n_total) *n_total = n;
    if (out && max_points > 0) std::memcpy(out, rp.data(), sizeof(double) * 3 * (size_t)(n < max_points ? n : max_points));
  });
}
int pmaf_get_dist_from_goal(pmaf_planner *h, double *out) {
  return guarded([&] {
    REQUIRE(h && out, "pmaf_get_dist_from_goal: NULL argument");
    // (goal_pos_ - real.getLatestPosition()).norm(), cf_manager.h:87-89, from the
    // host copy of the real position; same operation order as the device code
    const std::vector<double> &rp = h->real_pos_h;
    for (int p = 0; p < h->D.P; p++) {
      double dx = h->goal_h[p * 3] - rp[p * 3], dy = h->goal_h[p * 3 + 1] - rp[p * 3 + 1], dz = h->goal_h[p * 3 + 2] - rp[p * 3 + 2];
#ifdef PMAF_DOT_RIGHT_ASSOC
      out[p] = std::sqrt(dx * dx + (dy * dy + dz * dz));
#else
      out[p] = std::sqrt((dx * dx + dy * dy) + dz * dz);
#endif
    }
  });
}
int pmaf_get_best(pmaf_planner *h, int32_t *type, int32_t *id) {
  return guarded([&] {
    GETTER_PROLOGUE("pmaf_get_best")
    std::vector<int32_t> hb(D.P), bt(D.P), bi(D.P);
    h->download(hb.data(), D.has_best, D.P);
    h->download(bt.data(), D.best_type, D.P);
    h->download(bi.data(), D.best_id, D.P);
    for (int p = 0; p < D.P; p++) {
      if (type) type[p] = hb[p] ? bt[p] : -1;
      if (id) id[p] = hb[p] ? bi[p] : 0;
    }
  });
}
int pmaf_get_prediction_times_ns(pmaf_planner *h, double *out) {
  return guarded([&] {
    GETTER_PROLOGUE("pmaf_get_prediction_times_ns")
    REQUIRE(out, "NULL out");
    // per-agent device clock (wall_clock64: constant-rate counter, rate in kHz)
    int khz = 0;
    HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device));
    if (khz <= 0) khz = 100000;
    std::vector<unsigned long long> t(PN);
    h->download(t.data(), D.pred_ticks, PN);
    for (size_t i = 0; i < PN; i++) out[i] = (double)t[i] * (1e6 / (double)khz);
  });
}

int pmaf_set_best(pmaf_planner *h, const int32_t *id, const int32_t *type, const double *rand_vecs) {
  return guarded([&] {
    REQUIRE(h && id && type, "pmaf_set_best: NULL argument");
    h->use_device();
    sync(h);
    const DevView &D = h->D;
    std::vector<int32_t> hb(D.P);
    for (int p = 0; p < D.P; p++) {
      REQUIRE(id[p] >= 0 && id[p] <= D.N, "pmaf_set_best: id out of range");
      REQUIRE(id[p] == 0 || (type[p] >= PMAF_GOAL_HEURISTIC && type[p] <= PMAF_HAD_HEURISTIC),
              "pmaf_set_best: type must be one of the six heuristics when id > 0");
      hb[p] = id[p] > 0;
      if (p == 0) h->has_best_h = hb[p] ? 1 : 0;
    }
    h->upload(D.has_best, hb.data(), D.P);
    h->upload(D.best_id, id, D.P);
    h->upload(D.best_type, type, D.P);
    if (rand_vecs) {
      const int n_obs = D.n_obs;
      check_range(rand_vecs, (size_t)D.P * n_obs * 3, "pmaf_set_best: rand_vecs");
      std::vector<double> r((size_t)D.P * 3 * n_obs);
      for (int p = 0; p < D.P; p++)
        for (int i = 0; i < n_obs; i++)
          for (int c = 0; c < 3; c++) r[((size_t)p * 3 + c) * n_obs + i] = rand_vecs[((size_t)p * n_obs + i) * 3 + c];
      h->upload(D.best_rnd, r.data(), r.size());
    }
  });
}

int pmaf_get_tick_times_us(pmaf_planner *h, double *enqueue_us, double *setpoint_us, int32_t max_n, int32_t *n) {
  return guarded([&] {
    REQUIRE(h && n, "pmaf_get_tick_times_us: NULL argument");
    const size_t have = h->tick_count;
    const size_t k = (max_n > 0) ? std::min(have, (size_t)max_n) : 0;
    // oldest first among the newest k
    for (size_t i = 0; i < k; i++) {
      const size_t at = (h->tick_head + pmaf_planner::TICK_RING - k + i) % pmaf_planner::TICK_RING;
      if (enqueue_us) enqueue_us[i] = h->tick_enq_us[at];
      if (setpoint_us) setpoint_us[i] = h->tick_sp_us[at];
    }
    *n = (int32_t)k;
    h->tick_count = 0;
    h->tick_head = 0;
  });
}

// ---- failure detection / winner path (ABI 5) ----
int pmaf_get_health(pmaf_planner *h, int32_t *bits) {
  return guarded([&] {
    REQUIRE(h && bits, "pmaf_get_health: NULL argument");
    for (int p = 0; p < h->D.P; p++) bits[p] = (int32_t)h->mbox.host()[p * PMAF_MBOX + 15];   // (mailbox: host memory)
  });
}

int pmaf_debug_withhold_mailbox(pmaf_planner *h, int32_t enable) {
  return guarded([&] {
    REQUIRE(h, "pmaf_debug_withhold_mailbox: NULL handle");
    h->dbg_withhold = enable != 0;
  });
}

int pmaf_enable_winner_path(pmaf_planner *h, int32_t enable) {
  return guarded([&] {
    REQUIRE(h, "pmaf_enable_winner_path: NULL handle");
    h->use_device();
    sync(h);
    if (!enable) {
      h->wp.release();
      h->wph.release();
      h->wp_seq = 0.0;
      return;
    }
    if (h->wp.host()) return;
    const size_t P = (size_t)h->D.P;
    h->wph.alloc(sizeof(double) * P * 4);
    h->wp.alloc(sizeof(double) * P * h->D.cap * 3);   // (last: `wp` allocated is what "enabled" means)
    h->wp_np.assign(P, 0);
    h->wp_agent.assign(P, 0);
    h->wp_seq = 0.0;
    h->wp_timed = true;
  });
}

int pmaf_view_winner_path(pmaf_planner *h, const double **paths, const int32_t **n_points, const int32_t **agent) {
  return guarded([&] {
    REQUIRE(h, "pmaf_view_winner_path: NULL handle");
    if (!h->wp.host()) fail(PMAF_ERR_STATE, "pmaf_view_winner_path: not enabled (pmaf_enable_winner_path)");
    if (h->wp_seq == 0.0) fail(PMAF_ERR_STATE, "pmaf_view_winner_path: no selection yet (pmaf_tick / pmaf_evaluate), or the last "
                                               "tick's sequence number was withheld");
    // the path follows the set-point within microseconds (same kernel); bounded like the tick's own wait
    // (the stream is not asked, as it never was here: the tick's own wait has already seen this kernel publish)
    bounded_wait(
        SeqWords{h->wph.host() + 3, h->D.P, 4, h->wp_seq}, [] { return hipErrorNotReady; }, spin_pause, 1u << 14, h->tick_timeout_s,
        [] { fail(PMAF_ERR_DEVICE, "pmaf_view_winner_path: the path did not arrive within the time limit (PMAF_TICK_TIMEOUT_S)"); },
        "", "");
    if (!h->wp_timed) {
      h->wp_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h->last_tick_entry).count());
      if (h->wp_us.size() > (1u << 20)) h->wp_us.erase(h->wp_us.begin(), h->wp_us.begin() + (1u << 19));
      h->wp_timed = true;
    }
    for (int p = 0; p < h->D.P; p++) {
      h->wp_np[p] = (int32_t)h->wph.host()[p * 4];
      h->wp_agent[p] = (int32_t)h->wph.host()[p * 4 + 1];
    }
    if (paths) *paths = h->wp.host();
    if (n_points) *n_points = h->wp_np.data();
    if (agent) *agent = h->wp_agent.data();
  });
}

int pmaf_get_winner_path_times_us(pmaf_planner *h, double *out, int32_t max_n, int32_t *n) {
  return guarded([&] {
    REQUIRE(h && n, "pmaf_get_winner_path_times_us: NULL argument");
    std::vector<double> &v = h->wp_us;
    const size_t k = (out && max_n > 0) ? std::min(v.size(), (size_t)max_n) : 0;
    for (size_t i = 0; i < k; i++) out[i] = v[i];
    *n = (int32_t)k;
    v.clear();
  });
}

int pmaf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

void *pmaf_stream(pmaf_planner *h) { return h ? (void *)h->stream : nullptr; }

int pmaf_set_profiling(pmaf_planner *h, int32_t enable) {
  return guarded([&] {
    REQUIRE(h, "pmaf_set_profiling: NULL handle");
    h->use_device();
    sync(h);
    h->profiling = enable != 0;
    h->prof_every = enable > 1 ? enable : 1;
    h->prof_phase = 0;
  });
}
int pmaf_get_kernel_stats(pmaf_planner *h, double *rollout_ms, int64_t *launches, int64_t *agent_steps) {
  return guarded([&] {
    GETTER_PROLOGUE("pmaf_get_kernel_stats")
    if (rollout_ms) *rollout_ms = h->rollout_ms;
    if (launches) *launches = h->profiling ? h->timed_launches : h->launches;
    // (all launches since the reset, timed or not: pmaf_get_launch_count)
    if (agent_steps) {
      unsigned long long s = 0;
      h->download(&s, D.step_counter, 1);
      *agent_steps = (int64_t)s;
    }
  });
}
int pmaf_get_launch_count(pmaf_planner *h, int64_t *launches) {
  return guarded([&] {
    REQUIRE(h && launches, "pmaf_get_launch_count: NULL argument");
    *launches = h->launches;
  });
}
int pmaf_reset_kernel_stats(pmaf_planner *h) {
  return guarded([&] {
    REQUIRE(h, "pmaf_reset_kernel_stats: NULL handle");
    h->use_device();
    sync(h);
    h->rollout_ms = 0.0;
    h->launches = 0;
    h->timed_launches = 0;
    HIP_CHECK(hipMemsetAsync(h->D.step_counter, 0, sizeof(unsigned long long), h->stream));
    sync(h);
  });
}
int pmaf_debug_math(int32_t op, int32_t n, const double *a, const double *b, double *out) {
  return guarded([&] {
    REQUIRE(a && b && out && n > 0 && op >= 0 && op <= 20, "pmaf_debug_math: bad argument");
    DeviceBuf<double> bufs[3];   // (freed on every way out, a failed copy or launch included)
    for (auto &buf : bufs) buf.reserve(sizeof(double) * n);
    double *da = bufs[0].get(), *db = bufs[1].get(), *dout = bufs[2].get();
    HIP_CHECK(hipMemcpy(da, a, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(db, b, sizeof(double) * n, hipMemcpyHostToDevice));
    if (op <= 12) pmaf_k_launch_debug_math(op, n, da, db, dout, nullptr);
    else pmaf_k_launch_debug_math_ext(op, n, da, db, dout, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost));
  });
}

int pmaf_debug_external_rollout(pmaf_planner *h, const char *code_object_path, const char *kernel_name) {
  return guarded([&] {
    REQUIRE(h, "pmaf_debug_external_rollout: NULL handle");
    h->use_device();
    sync(h);
    if (h->ext_mod) { (void)hipModuleUnload(h->ext_mod); h->ext_mod = nullptr; h->ext_fn = nullptr; }
    h->route_in.external = false;
    reroute(h);
    if (!code_object_path) return;
    REQUIRE(kernel_name, "pmaf_debug_external_rollout: kernel name required");
    REQUIRE(h->route.lpa == 64, "pmaf_debug_external_rollout: wave-per-agent launches only (grid N x P, one wave per block)");
    HIP_CHECK(hipModuleLoad(&h->ext_mod, code_object_path));
    HIP_CHECK(hipModuleGetFunction(&h->ext_fn, h->ext_mod, kernel_name));
    h->route_in.external = true;
    reroute(h);
  });
}

int pmaf_get_launch_config(pmaf_planner *h, int32_t *lanes_per_agent, int32_t *n_blocks, int32_t *lds_bytes) {
  return guarded([&] {
    REQUIRE(h, "pmaf_get_launch_config: NULL handle");
    // (the one-wave figures for every handle: a MULTI_WAVE route's launcher asks for 96 KB on a grid of N x P itself
    // -- pmaf_k_mw.hip -- and this getter has always reported the one-wave kernel's blocks and bytes beside it)
    if (lanes_per_agent) *lanes_per_agent = h->route.lpa;
    if (n_blocks) *n_blocks = h->route.n_blocks * h->D.P;
    if (lds_bytes) *lds_bytes = (int32_t)h->route.lds_rollout;
  });
}

int pmaf_get_waves_per_agent(pmaf_planner *h, int32_t *waves_per_agent, int32_t *obstacles_per_wave) {
  return guarded([&] {
    REQUIRE(h, "pmaf_get_waves_per_agent: NULL handle");
    if (waves_per_agent) *waves_per_agent = h->route.waves;
    if (obstacles_per_wave) *obstacles_per_wave = h->route.per;
  });
}

int pmaf_get_priority_slices(pmaf_planner *h, int32_t *enabled, int32_t *slice_ticks, int32_t *younger_of_8) {
  return guarded([&] {
    REQUIRE(h, "pmaf_get_priority_slices: NULL handle");
    if (enabled) *enabled = h->route.sliced ? 1 : 0;
    if (slice_ticks) *slice_ticks = 1 << h->D.prio_slice_log2;
    if (younger_of_8) *younger_of_8 = h->D.prio_younger_of_8;
  });
}

int32_t pmaf_pick_lanes_per_agent(int32_t n_agents, int32_t n_populations, int32_t n_field_obstacles, int32_t n_simds) {
  if (n_agents < 1 || n_populations < 1 || n_field_obstacles < 0) return 0;
  return pmaf_route::pick_lpa(n_agents, n_populations, n_field_obstacles, n_simds > 0 ? n_simds : 1024);
}

double pmaf_estimate_rollout_us(int32_t lanes_per_agent, int32_t n_agents, int32_t n_populations, int32_t n_field_obstacles,
                                int32_t horizon, int32_t n_simds) {
  return pmaf_lpa::estimate_us(lanes_per_agent, n_agents, n_populations, n_field_obstacles, horizon, n_simds > 0 ? n_simds : 1024);
}

}  // extern "C"
