// pmaf_host_audit.cpp -- the calls that judge the predicted paths as they lie on the device, and their scratch: the
// obstacle distance, the path audit, the selection against the live list (pmaf_select_clear / pmaf_adopt_best), the six
// cross-audit calls, the joint selection, the link force. None of it runs inside pmaf_tick.
#include "pmaf_host_impl.hpp"
#include "pmaf_auditft.hpp"
#include "pmaf_xattach.hpp"
#include "pmaf_obstacle_slack.hpp"

extern "C" {

int pmaf_eval_obstacle_distance(pmaf_planner *h, const double *obstacles, double *out) {
  return guarded([&] {
    REQUIRE(h && obstacles && out, "pmaf_eval_obstacle_distance: NULL argument");
    h->use_device();
    sync(h);
    const double *d_obs = upload_plan_obstacles(h, obstacles);
    pmaf_k_launch_eval_obstacle_distance(h->D, d_obs, h->d_plan_out, h->stream);
    HIP_CHECK(hipGetLastError());
    h->download(out, h->d_plan_out, (size_t)h->D.P * h->D.N);
  });
}

// ---- path audit: the current predicted paths against a live obstacle list ----
// The reference declares CfManager::evaluatePath(const std::vector<Obstacle> &) (B/include/bimanual_planning_ros/
// cf_manager.h:130) without defining it, and evaluateAgents ignores its obstacle list (B/src/cf_manager.cpp:293-356).
// One implementation behind both exports: only_best = the selected agent of every population (outputs [P]).
// tracked (pmaf_evaluate_paths_tracked): the field obstacles of a population with tracks on the handle's resident
// tracks, read from `first` (NULL: the handle's offsets); the track buffer is then built by k_audit_track_ft.
struct TrackedCall {
  const int32_t *first;   // [P] or NULL
  const char *who;
};
static void check_tracked_first(const pmaf_planner *h, const TrackedCall &T);
static FTrackArgs tracked_args(pmaf_planner *h, const TrackedCall &T);
// the slacked calls against the live list (include/pmaf.h "clear selection with timing slack"): the arm up to `late`
// steps behind the obstacles' clock, the obstacles up to `early` behind the arm's. A null pointer is the call without
// slack; (0, 0) is a slacked call like any other and runs k_obs_slack_audit.
struct ObstacleSlack {
  int32_t late, early;
};
// host-side validation, before any wait. A slack of cap or more is clamped to cap here, before any device arithmetic
// (the contract's rule: then l < 2 cap on the device).
static ObstacleSlack clamp_obstacle_slack(const pmaf_planner *h, int32_t late, int32_t early, const std::string &who) {
  if (late < 0 || early < 0) fail(PMAF_ERR_INVALID, who + ": late and early must be >= 0");
  const int32_t cap = h->D.cap;
  return ObstacleSlack{late < cap ? late : cap, early < cap ? early : cap};
}

static void evaluate_paths(pmaf_planner *h, const double *obstacles, double margin, bool only_best, double *clearance,
                           int32_t *step, int32_t *obstacle, int32_t *first_violation, double *per_obstacle,
                           const TrackedCall *tracked = nullptr) {
  const DevView &D = h->D;
  const size_t n_obs = (size_t)D.n_obs, rows = only_best ? (size_t)D.P : (size_t)D.P * D.N;
  if (tracked) check_tracked_first(h, *tracked);
  check_range(obstacles, (size_t)D.P * n_obs * 7, "obstacles");
  check_range(&margin, 1, "margin");
  if ((size_t)D.cap * n_obs >= 0x7fffffffull) fail(PMAF_ERR_INVALID, "path audit: max_prediction_steps * n_obstacles must stay below 2^31");
  h->use_device();
  sync(h);   // behind the running rollout, like the getters of its results
  // device scratch: track | clearance [rows] | per_obstacle [rows][n_obs] | step, obstacle, first_violation [rows] each
  const size_t track_b = sizeof(double) * (size_t)D.P * D.cap * 3 * n_obs;
  const size_t full = (size_t)D.P * D.N;   // (sized for the all-agents call: both exports share the buffer)
  const size_t out_b = sizeof(double) * full + (per_obstacle ? sizeof(double) * full * n_obs : 0) + 3 * sizeof(int32_t) * full;
  h->d_audit.reserve(track_b + out_b);   // (track_b is the handle's: both grow exactly when out_b does)
  h->h_audit.reserve(out_b);
  char *d_out = h->d_audit.get() + track_b;
  AuditArgs A{};
  A.obs = upload_plan_obstacles(h, obstacles);
  A.track = reinterpret_cast<double *>(h->d_audit.get());
  A.margin = margin;
  A.only_best = only_best ? 1 : 0;
  while ((1 << A.group_log2) < D.n_obs && A.group_log2 < 6) A.group_log2++;
  size_t off = 0;
  A.clearance = reinterpret_cast<double *>(d_out + off); off += sizeof(double) * rows;
  if (per_obstacle) { A.per_obstacle = reinterpret_cast<double *>(d_out + off); off += sizeof(double) * rows * n_obs; }
  A.step = reinterpret_cast<int32_t *>(d_out + off); off += sizeof(int32_t) * rows;
  A.obstacle = reinterpret_cast<int32_t *>(d_out + off); off += sizeof(int32_t) * rows;
  A.first_violation = reinterpret_cast<int32_t *>(d_out + off); off += sizeof(int32_t) * rows;
  if (tracked && h->ftrk.on()) {   // (no tracks attached: the untracked launch, whose result it is)
    pmaf_k_launch_audit_track_ft(D, A.obs, tracked_args(h, *tracked), reinterpret_cast<double *>(h->d_audit.get()), h->stream);
    pmaf_k_launch_path_audit_only(D, A, h->stream);
  } else {
    pmaf_k_launch_path_audit(D, A, reinterpret_cast<double *>(h->d_audit.get()), h->stream);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h->h_audit.get(), d_out, off, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  const char *src = h->h_audit.get();
  std::memcpy(clearance, src, sizeof(double) * rows); src += sizeof(double) * rows;
  if (per_obstacle) { std::memcpy(per_obstacle, src, sizeof(double) * rows * n_obs); src += sizeof(double) * rows * n_obs; }
  int32_t *const outs[3] = {step, obstacle, first_violation};
  for (int32_t *o : outs) {
    if (o) std::memcpy(o, src, sizeof(int32_t) * rows);
    src += sizeof(int32_t) * rows;
  }
}

int pmaf_evaluate_paths(pmaf_planner *h, const double *obstacles, double margin, double *clearance, int32_t *step,
                        int32_t *obstacle, int32_t *first_violation, double *per_obstacle) {
  return guarded([&] {
    REQUIRE(h && obstacles && clearance, "pmaf_evaluate_paths: NULL argument");
    evaluate_paths(h, obstacles, margin, false, clearance, step, obstacle, first_violation, per_obstacle);
  });
}

int pmaf_evaluate_paths_tracked(pmaf_planner *h, const double *obstacles, const int32_t *first, double margin,
                                double *clearance, int32_t *step, int32_t *obstacle, int32_t *first_violation,
                                double *per_obstacle) {
  return guarded([&] {
    REQUIRE(h && obstacles && clearance, "pmaf_evaluate_paths_tracked: NULL argument");
    const TrackedCall T{first, "pmaf_evaluate_paths_tracked"};
    evaluate_paths(h, obstacles, margin, false, clearance, step, obstacle, first_violation, per_obstacle, &T);
  });
}

// the path audit with timing slack: the tracked audit's validation and staging (the list through
// upload_plan_obstacles, the call's offsets through tracked_args), then ONE kernel, k_obs_slack_audit, on the whole
// paths (horizon = cap) and every obstacle; its five outputs come back in one copy
int pmaf_evaluate_paths_slack(pmaf_planner *h, const double *obstacles, const int32_t *first, double margin, int32_t late,
                              int32_t early, double *clearance, int32_t *step, int32_t *obstacle_step, int32_t *obstacle,
                              int32_t *first_violation) {
  return guarded([&] {
    REQUIRE(h && obstacles && clearance, "pmaf_evaluate_paths_slack: NULL argument");
    const TrackedCall T{first, "pmaf_evaluate_paths_slack"};
    const DevView &D = h->D;
    const ObstacleSlack slack = clamp_obstacle_slack(h, late, early, T.who);
    check_tracked_first(h, T);
    check_range(obstacles, (size_t)D.P * D.n_obs * 7, "obstacles");
    check_range(&margin, 1, "margin");
    h->use_device();
    sync(h);   // behind the running rollout, like the getters of its results
    const size_t rows = (size_t)D.P * D.N;
    const size_t bytes = sizeof(double) * rows + 4 * sizeof(int32_t) * rows;
    h->d_oslack.reserve(bytes);
    h->h_oslack.reserve(bytes);
    ObsSlackArgs A{};
    A.obs = upload_plan_obstacles(h, obstacles);
    A.margin = margin;
    A.horizon = D.cap;
    A.n_audit = D.n_obs;
    A.late = slack.late;
    A.early = slack.early;
    char *d_out = h->d_oslack.get();
    A.clr = reinterpret_cast<double *>(d_out);
    int32_t *ints = reinterpret_cast<int32_t *>(d_out + sizeof(double) * rows);
    A.step = ints;
    A.obstacle_step = ints + rows;
    A.obstacle = ints + 2 * rows;
    A.fv = ints + 3 * rows;
    if (h->ftrk.on()) {   // (no tracks attached: every obstacle on the list's line)
      const FTrackArgs F = tracked_args(h, T);
      pmaf_k_launch_obs_slack_audit(D, A, &F, h->stream);
    } else {
      pmaf_k_launch_obs_slack_audit(D, A, nullptr, h->stream);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h->h_oslack.get(), d_out, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    const char *src = h->h_oslack.get();
    std::memcpy(clearance, src, sizeof(double) * rows); src += sizeof(double) * rows;
    int32_t *const outs[4] = {step, obstacle_step, obstacle, first_violation};
    for (int32_t *o : outs) {
      if (o) std::memcpy(o, src, sizeof(int32_t) * rows);
      src += sizeof(int32_t) * rows;
    }
  });
}

int pmaf_evaluate_path(pmaf_planner *h, const double *obstacles, double *clearance) {
  return guarded([&] {
    REQUIRE(h && obstacles && clearance, "pmaf_evaluate_path: NULL argument");
    h->use_device();
    if (h->has_best_h != 1 || h->D.P > 1) {   // (has_best_h speaks for population 0: read every population's flag back)
      sync(h);
      std::vector<int32_t> hb((size_t)h->D.P, 0);
      h->download(hb.data(), h->D.has_best, hb.size());
      if (h->has_best_h < 0) h->has_best_h = hb[0] ? 1 : 0;
      for (int32_t v : hb)
        if (!v) fail(PMAF_ERR_STATE, "pmaf_evaluate_path: no agent has been selected yet (call pmaf_evaluate / pmaf_tick first)");
    }
    evaluate_paths(h, obstacles, 0.0, true, clearance, nullptr, nullptr, nullptr, nullptr);
  });
}

// ---- selection against the live list (include/pmaf.h, "selection against the live list"): pmaf_select_clear,
// pmaf_adopt_best; kernels in pmaf_k_select.hip ----
// offset (in doubles) of the joint selection's result record in the select scratch's pinned area
static size_t select_pairclear_rec(const DevView &D) {
  return (size_t)D.P * 7 * D.n_obs + (size_t)D.P * PMAF_SELECT_REC + ((size_t)D.P + 1) / 2;
}

// ... and of the tracked calls' offsets behind it
static size_t select_tracked_first(const DevView &D) { return select_pairclear_rec(D) + PMAF_PAIRCLEAR_REC; }

static void select_scratch(pmaf_planner *h) {
  if (h->sel.host()) return;
  const DevView &D = h->D;
  const size_t list = (size_t)D.P * 7 * D.n_obs, PN = (size_t)D.P * D.N;
  h->d_sel_obs = h->dalloc_untracked<double>(list);
  h->d_sel_clr = h->dalloc_untracked<double>(PN);
  h->d_sel_fv = h->dalloc_untracked<int32_t>(PN);
  h->d_adopt_idx = h->dalloc_untracked<int32_t>((size_t)D.P);
  // list | result records [P] | previous picks [P] (int32, padded to a double) | the joint selection's record | the
  // tracked calls' offsets [P] (int32, padded)
  h->sel.alloc(sizeof(double) * (select_tracked_first(D) + ((size_t)D.P + 1) / 2));
}

// ---- the audits against the obstacle tracks (include/pmaf.h "audits against the obstacle tracks"): what the tracked
// calls add to the untracked ones' bodies; kernels in pmaf_k_auditft.hip ----
static void check_tracked_first(const pmaf_planner *h, const TrackedCall &T) {
  if (!T.first) return;
  for (int p = 0; p < h->D.P; p++) REQUIRE(T.first[p] >= 0, std::string(T.who) + ": first must be >= 0");
  if (!h->ftrk.on()) fail(PMAF_ERR_STATE, std::string(T.who) + ": no obstacle tracks are attached (pmaf_set_obstacle_tracks)");
}

// the handle's resident tracks as the kernels read them; the call's offsets travel like prev_idx, in mapped pinned
// memory (the caller has waited for the stream: no earlier call's kernel still reads the slot)
static FTrackArgs tracked_args(pmaf_planner *h, const TrackedCall &T) {
  const pmaf_planner::FieldTrack &f = h->ftrk;
  if (h->D.n_obs > PMAF_FTRACK_LANES) fail(PMAF_ERR_STATE, std::string(T.who) + ": obstacle tracks on a handle of more than 64 obstacles");
  FTrackArgs F{f.d_pts.get(), f.d_len.get(), f.d_first.get(), f.stride};
  if (T.first) {
    select_scratch(h);
    const size_t at = select_tracked_first(h->D);
    std::memcpy(h->sel.host() + at, T.first, sizeof(int32_t) * (size_t)h->D.P);
    F.first = reinterpret_cast<const int32_t *>(h->sel.dev() + at);
  }
  return F;
}

// Spin until a selection kernel has published `seq` in the last entry of each of `count` records of `rec_doubles`
// doubles (k_select_pick: one per population; k_pairclear_final: one); bounded like wait_mailbox, and an expired wait
// abandons the handle the same way (the kernels still read the scratch and may still adopt).
static void wait_select(pmaf_planner *h, const double *rec, int count, size_t rec_doubles, double seq, const char *who) {
  if (h->blocking_wait) HIP_CHECK(hipStreamSynchronize(h->stream));
  bounded_wait(
      SeqWords{rec + (rec_doubles - 1), count, rec_doubles, seq}, [&] { return hipStreamQuery(h->stream); }, spin_pause,
      1u << 14, h->tick_timeout_s,
      [&] {
        h->tick_abandoned = true;
        fail(PMAF_ERR_DEVICE, std::string(who) + ": no result from the selection kernel within the time limit (PMAF_TICK_TIMEOUT_S); "
                                                 "call pmaf_stop() before the next call");
      },
      who, ": the selection kernel finished without publishing its result");
}

// The obstacle side of every selection, clear or joint: the caller's list into the pinned scratch, the SelectArgs fields
// the audit reads, then k_select_stage and ONE audit in stream order -- k_select_audit; in a tracked call on a handle with
// tracks k_ft_select_audit (no tracks attached: the untracked audit, whose result it is); and k_ft_masked_audit where
// `ride` names columns of two populations' lists that the caller leaves to its pair side (bit j set = column j is NOT
// audited here). With `oslack` (pmaf_select_clear_slack) the one audit is k_obs_slack_audit, with or without tracks, into
// the same clr / fv. Returns the arguments, which a caller with a pick completes. Behind select_scratch().
static SelectArgs select_obstacle_side(pmaf_planner *h, const double *obstacles, double margin, int32_t horizon,
                                       bool skip_trailing, const TrackedCall *tracked, const AuditColumns *ride = nullptr,
                                       const ObstacleSlack *oslack = nullptr) {
  const DevView &D = h->D;
  aos_to_soa(obstacles, h->sel.host(), D.P, D.n_obs);
  SelectArgs A{};
  A.obs_src = h->sel.dev();
  A.obs = h->d_sel_obs;
  A.margin = margin;
  A.horizon = horizon < D.cap ? horizon : D.cap;   // (above the cap: the whole path)
  A.n_audit = skip_trailing ? D.n_obs - 1 : D.n_obs;   // (pmaf_select_clear: every obstacle counts, the trailing one included)
  A.clr = h->d_sel_clr;
  A.fv = h->d_sel_fv;
  const bool ft = tracked && h->ftrk.on();
  FTrackArgs F{};
  if (ft) F = tracked_args(h, *tracked);
  pmaf_k_launch_select_stage(D, A, h->stream);
  if (oslack) {
    ObsSlackArgs O{};
    O.obs = A.obs;
    O.margin = A.margin;
    O.horizon = A.horizon;
    O.n_audit = A.n_audit;
    O.late = oslack->late;
    O.early = oslack->early;
    O.clr = A.clr;
    O.fv = A.fv;
    pmaf_k_launch_obs_slack_audit(D, O, ft ? &F : nullptr, h->stream);
  } else if (!ft) {
    pmaf_k_launch_select_audit(D, A, h->stream);
  } else if (ride && (ride->cols_a | ride->cols_b) != 0) {
    const uint64_t all = A.n_audit >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << A.n_audit) - 1;
    const AuditColumns audited{ride->pop_a, ride->pop_b, all & ~ride->cols_a, all & ~ride->cols_b};
    pmaf_k_launch_select_audit_ft(D, A, F, &audited, h->stream);
  } else {
    pmaf_k_launch_select_audit_ft(D, A, F, nullptr, h->stream);
  }
  HIP_CHECK(hipGetLastError());
  return A;
}

// One body behind pmaf_select_clear, pmaf_select_clear_tracked (tracked != NULL; n_audit = n_obs, or n_obs - 1 when
// the tracked call skips the trailing obstacle) and pmaf_select_clear_slack (tracked and oslack != NULL). Called inside
// guarded().
static void select_clear(pmaf_planner *h, const double *obstacles, double margin, int32_t horizon, const int32_t *prev_idx,
                         int32_t adopt, int32_t *pick, int32_t *rule, int32_t *n_clear, double *cost, double *clearance,
                         int32_t *first_violation, const std::string &who, const TrackedCall *tracked, bool skip_trailing,
                         const ObstacleSlack *oslack = nullptr) {
  REQUIRE(h && obstacles && pick, who + ": NULL argument");
  const DevView &D = h->D;
  REQUIRE(horizon >= 1, who + ": horizon must be >= 1");
  if (prev_idx)
    for (int p = 0; p < D.P; p++) REQUIRE(prev_idx[p] >= -1 && prev_idx[p] < D.N, who + ": prev_idx out of range");
  if (tracked) check_tracked_first(h, *tracked);
  check_range(obstacles, (size_t)D.P * D.n_obs * 7, "obstacles");
  check_range(&margin, 1, "margin");
  h->use_device();
  require_drained(h, who.c_str());
  sync(h);   // behind the running rollout, like the getters of its results
  select_scratch(h);
  const size_t list = (size_t)D.P * 7 * D.n_obs;
  double *rec = h->sel.host() + list;
  int32_t *prev_h = reinterpret_cast<int32_t *>(rec + (size_t)D.P * PMAF_SELECT_REC);
  if (prev_idx) std::memcpy(prev_h, prev_idx, sizeof(int32_t) * (size_t)D.P);
  SelectArgs A = select_obstacle_side(h, obstacles, margin, horizon, skip_trailing, tracked, nullptr, oslack);
  A.adopt = adopt ? 1 : 0;
  A.prev = prev_idx ? reinterpret_cast<const int32_t *>(h->sel.dev() + list + (size_t)D.P * PMAF_SELECT_REC) : nullptr;
  A.result = h->sel.dev() + list;
  A.seq = (h->sel_seq += 1.0);
  pmaf_k_launch_select_pick(D, A, h->stream);
  HIP_CHECK(hipGetLastError());
  wait_select(h, rec, D.P, PMAF_SELECT_REC, A.seq, who.c_str());
  if (adopt) h->has_best_h = 1;
  for (int p = 0; p < D.P; p++) {
    const double *r = rec + (size_t)p * PMAF_SELECT_REC;
    pick[p] = (int32_t)r[0];
    if (rule) rule[p] = (int32_t)r[1];
    if (n_clear) n_clear[p] = (int32_t)r[2];
    if (first_violation) first_violation[p] = (int32_t)r[3];
    if (cost) cost[p] = r[4];
    if (clearance) clearance[p] = r[5];
  }
}

int pmaf_select_clear(pmaf_planner *h, const double *obstacles, double margin, int32_t horizon, const int32_t *prev_idx,
                      int32_t adopt, int32_t *pick, int32_t *rule, int32_t *n_clear, double *cost, double *clearance,
                      int32_t *first_violation) {
  return guarded([&] {
    select_clear(h, obstacles, margin, horizon, prev_idx, adopt, pick, rule, n_clear, cost, clearance, first_violation,
                 "pmaf_select_clear", nullptr, false);
  });
}

int pmaf_select_clear_tracked(pmaf_planner *h, const double *obstacles, const int32_t *first, double margin, int32_t horizon,
                              int32_t skip_trailing, const int32_t *prev_idx, int32_t adopt, int32_t *pick, int32_t *rule,
                              int32_t *n_clear, double *cost, double *clearance, int32_t *first_violation) {
  return guarded([&] {
    const TrackedCall T{first, "pmaf_select_clear_tracked"};
    select_clear(h, obstacles, margin, horizon, prev_idx, adopt, pick, rule, n_clear, cost, clearance, first_violation,
                 T.who, &T, skip_trailing != 0);
  });
}

int pmaf_select_clear_slack(pmaf_planner *h, const double *obstacles, const int32_t *first, double margin, int32_t horizon,
                            int32_t skip_trailing, int32_t late, int32_t early, const int32_t *prev_idx, int32_t adopt,
                            int32_t *pick, int32_t *rule, int32_t *n_clear, double *cost, double *clearance,
                            int32_t *first_violation) {
  return guarded([&] {
    const TrackedCall T{first, "pmaf_select_clear_slack"};
    REQUIRE(h && obstacles && pick, std::string(T.who) + ": NULL argument");
    const ObstacleSlack slack = clamp_obstacle_slack(h, late, early, T.who);
    select_clear(h, obstacles, margin, horizon, prev_idx, adopt, pick, rule, n_clear, cost, clearance, first_violation,
                 T.who, &T, skip_trailing != 0, &slack);
  });
}

int pmaf_adopt_best(pmaf_planner *h, const int32_t *agent_idx) {
  return guarded([&] {
    REQUIRE(h && agent_idx, "pmaf_adopt_best: NULL argument");
    const DevView &D = h->D;
    for (int p = 0; p < D.P; p++) REQUIRE(agent_idx[p] >= -1 && agent_idx[p] < D.N, "pmaf_adopt_best: agent_idx out of range");
    h->use_device();
    require_drained(h, "pmaf_adopt_best");
    AdoptArgs A{};
    if (D.P <= PMAF_ADOPT_INLINE) {   // by value in the kernel arguments: nothing for a later call to overwrite
      for (int p = 0; p < D.P; p++) A.idx_val[p] = agent_idx[p];
    } else {
      select_scratch(h);
      HIP_CHECK(hipStreamSynchronize(h->stream));   // (an earlier call's kernel may still read d_adopt_idx)
      h->upload(h->d_adopt_idx, agent_idx, (size_t)D.P);
      A.idx = h->d_adopt_idx;
    }
    pmaf_k_launch_adopt_best(D, A, h->stream);   // enqueued: ordered in front of the next manager launch by the stream
    HIP_CHECK(hipGetLastError());
    if (agent_idx[0] >= 0) h->has_best_h = 1;   // (has_best_h speaks for population 0)
  });
}

// ---- cross audit: two path sets against each other; the pair pick (include/pmaf.h, "cross audit" and "cross audit with
// timing slack"). Six calls, one path: a call is "population against population" or "population against uploaded
// tracks", step against step (k_cross_audit) or slacked (k_cross_audit_slack), and a select call adds the pair pick ----
// a slacked call's two slacks. A null pointer is the step-against-step audit; a slack of (0, 0) is a slacked call like
// any other and runs k_cross_audit_slack.
struct XAuditSlack {
  int32_t late_a, late_b;
};
// Device scratch of one call: clearance [n_a][n_b] | partials | result | tracks [n_tracks][cap][3] | step [n_a][n_b] |
// track lengths [n_tracks] | the slacked calls' second step matrix [n_a][n_b] | the joint selection's parts: partials |
// track costs [n_tracks] | windowed lengths [n_a], [n_b] (doubles first, the int32 parts padded: every part stays 8-byte
// aligned) | the slacked attached audit's sphere matrix [n_a][n_b] (LAST: no other call's layout moves with it)
struct XAuditBuf {
  double *clearance;
  PairBest *partial;
  PairResult *result;
  double *tracks;
  int32_t *step, *track_len;
  int32_t *step_b;   // (the slacked calls only)
  // (the joint selection only)
  PairClearBest *pc_partial;
  double *track_cost;
  int32_t *win_a, *win_b;
  int32_t *sphere;   // (the slacked attached audit only: the attached audit keeps its sphere matrix where step_b lies)
};
// the joint selection's audit window: the cross audit then runs on the lengths min(n, horizon) (k_pairclear_window), its
// matrix stays in the scratch, and nothing is copied out
struct XAuditWindow {
  int32_t horizon;   // 1 .. cap
};
static XAuditBuf xaudit_scratch(pmaf_planner *h, size_t n_a, size_t n_b, size_t n_tracks, bool two_steps, bool joint = false,
                                bool third = false) {
  const size_t pairs = n_a * n_b;
  if (pairs >= 0x7fffffffull) fail(PMAF_ERR_INVALID, "cross audit: the number of pairs must stay below 2^31");
  const size_t b_clr = sizeof(double) * pairs, b_part = sizeof(PairBest) * PMAF_XAUDIT_PARTIALS, b_res = sizeof(PairResult);
  const size_t b_trk = sizeof(double) * n_tracks * (size_t)h->D.cap * 3, b_step = (sizeof(int32_t) * pairs + 7) & ~(size_t)7;
  const size_t b_len = (sizeof(int32_t) * n_tracks + 7) & ~(size_t)7;
  const size_t b_pc = sizeof(PairClearBest) * PMAF_XAUDIT_PARTIALS, b_tc = sizeof(double) * n_tracks;
  const size_t b_wa = (sizeof(int32_t) * n_a + 7) & ~(size_t)7, b_wb = (sizeof(int32_t) * n_b + 7) & ~(size_t)7;
  const size_t total = b_clr + b_part + b_res + b_trk + b_step + b_len + (two_steps ? b_step : 0) +
                       (joint ? b_pc + b_tc + b_wa + b_wb : 0) + (third ? b_step : 0);
  h->d_xaudit.reserve(total);
  XAuditBuf B;
  char *p = h->d_xaudit.get();
  B.clearance = reinterpret_cast<double *>(p); p += b_clr;
  B.partial = reinterpret_cast<PairBest *>(p); p += b_part;
  B.result = reinterpret_cast<PairResult *>(p); p += b_res;
  B.tracks = reinterpret_cast<double *>(p); p += b_trk;
  B.step = reinterpret_cast<int32_t *>(p); p += b_step;
  B.track_len = reinterpret_cast<int32_t *>(p); p += b_len;
  B.step_b = two_steps ? reinterpret_cast<int32_t *>(p) : nullptr;
  if (two_steps) p += b_step;
  B.pc_partial = joint ? reinterpret_cast<PairClearBest *>(p) : nullptr; p += joint ? b_pc : 0;
  B.track_cost = joint ? reinterpret_cast<double *>(p) : nullptr; p += joint ? b_tc : 0;
  B.win_a = joint ? reinterpret_cast<int32_t *>(p) : nullptr; p += joint ? b_wa : 0;
  B.win_b = joint ? reinterpret_cast<int32_t *>(p) : nullptr; p += joint ? b_wb : 0;
  B.sphere = third ? reinterpret_cast<int32_t *>(p) : nullptr;
  return B;
}

// host-side validation of a slacked call's slacks, before any wait. A slack of cap or more already admits every pair of
// steps: clamped here, before any device arithmetic.
static void clamp_slack(const pmaf_planner *h, XAuditSlack *slack, const char *who) {
  if (!slack) return;
  for (int32_t *late : {&slack->late_a, &slack->late_b}) {
    if (*late < 0) fail(PMAF_ERR_INVALID, std::string(who) + ": late_a and late_b must be >= 0");
    *late = *late < h->D.cap ? *late : h->D.cap;
  }
}

// the attached audit (include/pmaf.h "joint selection on coupled handles"): the two populations whose lists' spheres
// ride on each other's candidate paths, and the staged list [P][7][n_obs] on the device whose radii the terms take. The
// terms themselves are the coupling's resident rows (pmaf_planner::FieldTrack::d_src / d_scale / d_anchor): nothing is
// uploaded for the call. The sphere matrix, when wanted, lies where the slacked calls keep their second step matrix; a call
// with a slack AND an attachment (pmaf_cross_audit_attached_slack, the pair side of pmaf_select_pair_clear_tracked_slack)
// wants both, and its sphere matrix is XAuditBuf::sphere, the last part of the scratch.
struct XAuditAttach {
  int32_t pop_a, pop_b;
  const double *list;
  bool want_sphere;
};
// the columns of population p's list that ride on population q's path in the handle's CURRENT coupling, as a mask
static uint64_t attached_columns(const pmaf_planner *h, int32_t p, int32_t q) {
  const pmaf_planner::FieldTrack &f = h->ftrk;
  if (!f.coupled) return 0;
  const int M = h->D.n_obs - 1;
  uint64_t m = 0;
  for (int s = 0; s < M && s < PMAF_FTRACK_LANES; s++)
    if (f.src[(size_t)p * M + s] == q) m |= (uint64_t)1 << s;
  return m;
}
static XAttachSide attach_side(const pmaf_planner *h, const XAuditAttach &T, int32_t p) {
  const pmaf_planner::FieldTrack &f = h->ftrk;
  const double *rad = T.list + ((size_t)p * 7 + 6) * h->D.n_obs;
  if (!f.coupled) return XAttachSide{nullptr, nullptr, nullptr, rad};
  return XAttachSide{f.d_src.get() + (size_t)p * PMAF_FTRACK_LANES, f.d_scale.get() + (size_t)p * PMAF_FTRACK_LANES,
                     f.d_anchor.get() + (size_t)p * 3 * PMAF_FTRACK_LANES, rad};
}
// the attached kernels' arguments: the cross audit's X and the two populations' terms; sphere: where the call's sphere
// matrix lies in the scratch (XAuditAttach above)
static CrossAuditAttachedArgs attached_args(const pmaf_planner *h, const CrossAuditArgs &X, const XAuditAttach &att,
                                            int32_t *sphere) {
  CrossAuditAttachedArgs T{};
  T.X = X;
  T.a = attach_side(h, att, att.pop_a);
  T.b = attach_side(h, att, att.pop_b);
  T.pop_a = att.pop_a;
  T.pop_b = att.pop_b;
  T.M = h->D.n_obs - 1;
  T.radius = h->D.C.rad;
  T.sphere = att.want_sphere ? sphere : nullptr;
  return T;
}

// the launch: set A against set B into the scratch, the step matrices where they are wanted. Four kernels: step against
// step or slacked, each with or without the attached terms
static void xaudit_launch(pmaf_planner *h, const XAuditBuf &B, const double *paths_a, const int32_t *len_a, int32_t n_a,
                          const double *paths_b, const int32_t *len_b, int32_t n_b, double separation,
                          const XAuditSlack *slack, bool want_a, bool want_b, const XAuditWindow *win = nullptr,
                          const XAuditAttach *att = nullptr) {
  if (win) {   // both sides cut to their windows: the audit kernels read these lengths instead
    PairWindowArgs W{};
    W.n_a = len_a;
    W.n_b = len_b;
    W.count_a = n_a;
    W.count_b = n_b;
    W.cap = h->D.cap;
    W.horizon = win->horizon;
    W.len_a = B.win_a;
    W.len_b = B.win_b;
    pmaf_k_launch_pairclear_window(W, h->stream);
    len_a = B.win_a;
    len_b = B.win_b;
  }
  CrossAuditSlackArgs S{};
  CrossAuditArgs &A = S.X;
  A.paths_a = paths_a;
  A.paths_b = paths_b;
  A.len_a = len_a;
  A.len_b = len_b;
  A.n_a = n_a;
  A.n_b = n_b;
  A.cap = h->D.cap;
  A.separation = separation;
  A.clearance = B.clearance;
  A.step = want_a ? B.step : nullptr;
  if (slack && att) {   // the attached audit's terms over the slacked audit's band
    CrossAuditAttachedSlackArgs U{};
    U.T = attached_args(h, A, *att, B.sphere);
    U.late_a = slack->late_a;
    U.late_b = slack->late_b;
    U.step_b = want_b ? B.step_b : nullptr;
    pmaf_k_launch_cross_audit_attached_slack(U, h->stream);
  } else if (slack) {
    S.late_a = slack->late_a;
    S.late_b = slack->late_b;
    S.step_b = want_b ? B.step_b : nullptr;
    pmaf_k_launch_cross_audit_slack(S, h->stream);
  } else if (att) {
    pmaf_k_launch_cross_audit_attached(attached_args(h, A, *att, B.step_b), h->stream);
  } else {
    pmaf_k_launch_cross_audit(A, h->stream);
  }
  HIP_CHECK(hipGetLastError());
}

// the matrix (and the step matrices the caller asked for) back to the host
static void xaudit_download(pmaf_planner *h, const XAuditBuf &B, size_t pairs, double *clearance, int32_t *step_a,
                            int32_t *step_b, int32_t *sphere = nullptr) {
  if (sphere) HIP_CHECK(hipMemcpyAsync(sphere, B.sphere, sizeof(int32_t) * pairs, hipMemcpyDeviceToHost, h->stream));
  if (step_a) HIP_CHECK(hipMemcpyAsync(step_a, B.step, sizeof(int32_t) * pairs, hipMemcpyDeviceToHost, h->stream));
  if (step_b) HIP_CHECK(hipMemcpyAsync(step_b, B.step_b, sizeof(int32_t) * pairs, hipMemcpyDeviceToHost, h->stream));
  h->download(clearance, B.clearance, pairs);
}

// population pop_a's paths against population pop_b's where they lie; the matrix stays in the scratch
static XAuditBuf cross_audit_populations(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, XAuditSlack *slack,
                                         bool want_a, bool want_b, const char *who, const XAuditWindow *win = nullptr,
                                         const XAuditAttach *att = nullptr) {
  const DevView &D = h->D;
  if (pop_a < 0 || pop_a >= D.P || pop_b < 0 || pop_b >= D.P || pop_a == pop_b)
    fail(PMAF_ERR_INVALID, std::string(who) + ": need two different populations of the handle");
  check_range(&separation, 1, "separation");
  clamp_slack(h, slack, who);
  h->use_device();
  if (!win) sync(h);   // behind the running rollout, like the getters of its results (the joint selection has waited)
  const XAuditBuf B = xaudit_scratch(h, (size_t)D.N, (size_t)D.N, 0, slack != nullptr || (att && att->want_sphere), win != nullptr,
                                     slack != nullptr && att && att->want_sphere);
  xaudit_launch(h, B, D.paths + (size_t)pop_a * D.N * D.cap * 3, D.n_points + (size_t)pop_a * D.N, D.N,
                D.paths + (size_t)pop_b * D.N * D.cap * 3, D.n_points + (size_t)pop_b * D.N, D.N, separation, slack, want_a,
                want_b, win, att);
  return B;
}

// population pop's paths against the caller's tracks, uploaded into the scratch; the results back to the host (the
// joint selection: no clearance pointer, the matrix stays in the scratch; step_a / step_b then only say which step
// matrices to keep, and track_cost [n_tracks] or NULL is uploaded beside the tracks)
static XAuditBuf cross_audit_tracks(pmaf_planner *h, int32_t pop, int32_t n_tracks, const double *tracks,
                                    const int32_t *n_track_points, double separation, XAuditSlack *slack, double *clearance,
                                    int32_t *step_a, int32_t *step_b, const char *who, const XAuditWindow *win = nullptr,
                                    const double *track_cost = nullptr) {
  const DevView &D = h->D;
  REQUIRE(pop >= 0 && pop < D.P, std::string(who) + ": population out of range");
  REQUIRE(n_tracks > 0, std::string(who) + ": n_tracks must be > 0");
  check_range(&separation, 1, "separation");
  clamp_slack(h, slack, who);
  // rows past a track's count are neither checked nor copied
  const size_t row = (size_t)D.cap * 3;
  std::vector<double> packed((size_t)n_tracks * row, 0.0);
  for (int32_t t = 0; t < n_tracks; t++) {
    REQUIRE(n_track_points[t] >= 0 && n_track_points[t] <= D.cap, std::string(who) + ": a track's point count must be in [0, max_prediction_steps]");
    check_range(tracks + t * row, (size_t)n_track_points[t] * 3, "tracks");
    std::memcpy(packed.data() + t * row, tracks + t * row, sizeof(double) * 3 * (size_t)n_track_points[t]);
  }
  h->use_device();
  if (!win) sync(h);
  const XAuditBuf B = xaudit_scratch(h, (size_t)D.N, (size_t)n_tracks, (size_t)n_tracks, slack != nullptr, win != nullptr);
  HIP_CHECK(hipMemcpyAsync(B.track_len, n_track_points, sizeof(int32_t) * (size_t)n_tracks, hipMemcpyHostToDevice, h->stream));
  if (track_cost) HIP_CHECK(hipMemcpyAsync(B.track_cost, track_cost, sizeof(double) * (size_t)n_tracks, hipMemcpyHostToDevice, h->stream));
  h->upload(B.tracks, packed.data(), packed.size());
  xaudit_launch(h, B, D.paths + (size_t)pop * D.N * D.cap * 3, D.n_points + (size_t)pop * D.N, D.N, B.tracks, B.track_len,
                n_tracks, separation, slack, step_a != nullptr, step_b != nullptr, win);
  if (clearance) xaudit_download(h, B, (size_t)D.N * n_tracks, clearance, step_a, step_b);
  return B;
}

// the pair pick over the matrix cross_audit_populations left in the scratch. The costs are read where pmaf_get_costs
// reads them (DevView::costs, behind the same wait), so both calls see the same values in every state of the handle.
static void select_pair(pmaf_planner *h, const XAuditBuf &B, int32_t pop_a, int32_t pop_b, double margin, int32_t *pair,
                        double *pair_cost, double *pair_clearance, int32_t *feasible) {
  const DevView &D = h->D;
  PairArgs A{};
  A.clearance = B.clearance;
  A.cost_a = D.costs + (size_t)pop_a * D.N;
  A.cost_b = D.costs + (size_t)pop_b * D.N;
  A.n_a = A.n_b = D.N;
  A.margin = margin;
  A.partial = B.partial;
  A.result = B.result;
  pmaf_k_launch_pair_reduce(A, h->stream);
  HIP_CHECK(hipGetLastError());
  PairResult r{};
  h->download(&r, B.result, 1);
  pair[0] = r.i; pair[1] = r.j;
  *pair_cost = r.cost;
  *pair_clearance = r.clearance;
  *feasible = r.feasible;
}

int pmaf_cross_audit(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, double *clearance, int32_t *step) {
  return guarded([&] {
    REQUIRE(h && clearance, "pmaf_cross_audit: NULL argument");
    const XAuditBuf B = cross_audit_populations(h, pop_a, pop_b, separation, nullptr, step != nullptr, false, "pmaf_cross_audit");
    xaudit_download(h, B, (size_t)h->D.N * h->D.N, clearance, step, nullptr);
  });
}

// what pmaf_cross_audit_attached and its slacked form do before the audit: the arguments' validation (all of it before any
// wait), then the list staged on the device behind the running rollout
static XAuditAttach attached_prologue(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles, double separation,
                                      XAuditSlack *slack, const double *clearance, bool want_sphere, const char *who) {
  REQUIRE(h && obstacles && clearance, std::string(who) + ": NULL argument");
  const DevView &D = h->D;
  if (pop_a < 0 || pop_a >= D.P || pop_b < 0 || pop_b >= D.P || pop_a == pop_b)
    fail(PMAF_ERR_INVALID, std::string(who) + ": need two different populations of the handle");
  check_range(&separation, 1, "separation");
  clamp_slack(h, slack, who);
  check_range(obstacles, (size_t)D.P * D.n_obs * 7, "obstacles");
  h->use_device();
  sync(h);   // behind the running rollout; the list's upload below is in stream order behind it
  return XAuditAttach{pop_a, pop_b, upload_plan_obstacles(h, obstacles), want_sphere};
}

int pmaf_cross_audit_attached(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles, double separation,
                              double *clearance, int32_t *step, int32_t *sphere) {
  return guarded([&] {
    const char *who = "pmaf_cross_audit_attached";
    const XAuditAttach T = attached_prologue(h, pop_a, pop_b, obstacles, separation, nullptr, clearance, sphere != nullptr, who);
    const XAuditBuf B = cross_audit_populations(h, pop_a, pop_b, separation, nullptr, step != nullptr, false, who, nullptr, &T);
    xaudit_download(h, B, (size_t)h->D.N * h->D.N, clearance, step, sphere);   // (the sphere matrix lies in the step_b part)
  });
}

int pmaf_cross_audit_attached_slack(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles, double separation,
                                    int32_t late_a, int32_t late_b, double *clearance, int32_t *step_a, int32_t *step_b,
                                    int32_t *sphere) {
  return guarded([&] {
    const char *who = "pmaf_cross_audit_attached_slack";
    XAuditSlack slack{late_a, late_b};
    const XAuditAttach T = attached_prologue(h, pop_a, pop_b, obstacles, separation, &slack, clearance, sphere != nullptr, who);
    const XAuditBuf B = cross_audit_populations(h, pop_a, pop_b, separation, &slack, step_a != nullptr, step_b != nullptr, who,
                                                nullptr, &T);
    xaudit_download(h, B, (size_t)h->D.N * h->D.N, clearance, step_a, step_b, sphere);
  });
}

int pmaf_cross_audit_tracks(pmaf_planner *h, int32_t pop, int32_t n_tracks, const double *tracks,
                            const int32_t *n_track_points, double separation, double *clearance, int32_t *step) {
  return guarded([&] {
    REQUIRE(h && tracks && n_track_points && clearance, "pmaf_cross_audit_tracks: NULL argument");
    cross_audit_tracks(h, pop, n_tracks, tracks, n_track_points, separation, nullptr, clearance, step, nullptr,
                       "pmaf_cross_audit_tracks");
  });
}

int pmaf_select_pair(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, double margin, int32_t *pair,
                     double *pair_cost, double *pair_clearance, int32_t *feasible) {
  return guarded([&] {
    REQUIRE(h && pair && pair_cost && pair_clearance && feasible, "pmaf_select_pair: NULL argument");
    check_range(&margin, 1, "margin");
    const XAuditBuf B = cross_audit_populations(h, pop_a, pop_b, separation, nullptr, false, false, "pmaf_select_pair");
    select_pair(h, B, pop_a, pop_b, margin, pair, pair_cost, pair_clearance, feasible);
  });
}

int pmaf_cross_audit_slack(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, int32_t late_a, int32_t late_b,
                           double *clearance, int32_t *step_a, int32_t *step_b) {
  return guarded([&] {
    REQUIRE(h && clearance, "pmaf_cross_audit_slack: NULL argument");
    XAuditSlack slack{late_a, late_b};
    const XAuditBuf B = cross_audit_populations(h, pop_a, pop_b, separation, &slack, step_a != nullptr, step_b != nullptr,
                                                "pmaf_cross_audit_slack");
    xaudit_download(h, B, (size_t)h->D.N * h->D.N, clearance, step_a, step_b);
  });
}

int pmaf_cross_audit_tracks_slack(pmaf_planner *h, int32_t pop, int32_t n_tracks, const double *tracks,
                                  const int32_t *n_track_points, double separation, int32_t late_a, int32_t late_b,
                                  double *clearance, int32_t *step_a, int32_t *step_b) {
  return guarded([&] {
    REQUIRE(h && tracks && n_track_points && clearance, "pmaf_cross_audit_tracks_slack: NULL argument");
    XAuditSlack slack{late_a, late_b};
    cross_audit_tracks(h, pop, n_tracks, tracks, n_track_points, separation, &slack, clearance, step_a, step_b,
                       "pmaf_cross_audit_tracks_slack");
  });
}

int pmaf_select_pair_slack(pmaf_planner *h, int32_t pop_a, int32_t pop_b, double separation, double margin, int32_t late_a,
                           int32_t late_b, int32_t *pair, double *pair_cost, double *pair_clearance, int32_t *feasible,
                           int32_t *pair_steps) {
  return guarded([&] {
    REQUIRE(h && pair && pair_cost && pair_clearance && feasible, "pmaf_select_pair_slack: NULL argument");
    check_range(&margin, 1, "margin");
    XAuditSlack slack{late_a, late_b};
    const XAuditBuf B = cross_audit_populations(h, pop_a, pop_b, separation, &slack, pair_steps != nullptr,
                                                pair_steps != nullptr, "pmaf_select_pair_slack");
    select_pair(h, B, pop_a, pop_b, margin, pair, pair_cost, pair_clearance, feasible);
    if (pair_steps) {   // the two steps of the returned pair's matrix entry
      pair_steps[0] = pair_steps[1] = -1;
      if (pair[0] >= 0 && pair[1] >= 0) {
        const size_t o = (size_t)pair[0] * h->D.N + pair[1];
        h->download(pair_steps, B.step + o, 1);
        h->download(pair_steps + 1, B.step_b + o, 1);
      }
    }
  });
}

// ---- joint selection (include/pmaf.h, "joint selection: clear of the live list and of each other"):
// pmaf_select_pair_clear, pmaf_select_clear_tracks. One path for both: the select path's audit (k_select_stage,
// k_select_audit into its scratch), the cross audit path above with a window, then pmaf_k_pairclear.hip's reduction over
// what both left on the device. Side B is population pop_b, or -- pop_b < 0 -- the caller's tracks.
// pmaf_select_pair_clear_tracked (include/pmaf.h, "joint selection on coupled handles") is the same path with a
// TrackedCall: the obstacle side is then the tracked selection's audit (k_ft_select_audit, or k_ft_masked_audit where
// columns of either list ride on the other member of the pair) and the pair side k_cross_audit_attached; a handle
// without tracks and without such columns launches exactly what pmaf_select_pair_clear launches.
// pmaf_select_pair_clear_tracked_slack passes `late` as well: the pair side is then k_xaudit_attached_slack where columns
// ride on the other member, and k_cross_audit_slack where none does. ----
struct PairClearSideB {
  int32_t pop_b, n_tracks;
  const double *tracks;
  const int32_t *n_track_points;
  const double *track_cost;
};
struct PairClearOut {
  int32_t *pair, *rule, *n_feasible, *n_clear;
  double *pair_cost, *pair_clearance, *obstacle_clearance;
  int32_t *first_violation;
  double *worst_excess;
  int32_t *pair_steps;
};
static void select_pair_clear(pmaf_planner *h, int32_t pop_a, const PairClearSideB &sb, const double *obstacles,
                              double obstacle_margin, int32_t horizon, int32_t skip_trailing, double separation,
                              double pair_margin, const int32_t *late, const int32_t *prev_pair, int32_t adopt,
                              const PairClearOut &out, const std::string &who, const TrackedCall *tracked = nullptr) {
  const DevView &D = h->D;
  const bool tracks = sb.pop_b < 0;
  REQUIRE(horizon >= 1, who + ": horizon must be >= 1");
  REQUIRE(pop_a >= 0 && pop_a < D.P, who + ": population out of range");
  if (!tracks && (sb.pop_b >= D.P || sb.pop_b == pop_a)) fail(PMAF_ERR_INVALID, who + ": need two different populations of the handle");
  if (tracks) REQUIRE(sb.n_tracks > 0, who + ": n_tracks must be > 0");
  const int32_t n_b = tracks ? sb.n_tracks : D.N;
  if (prev_pair)
    REQUIRE(prev_pair[0] >= -1 && prev_pair[0] < D.N && prev_pair[1] >= -1 && prev_pair[1] < n_b, who + ": prev_pair out of range");
  XAuditSlack slack{0, 0};
  if (late) slack = XAuditSlack{late[0], late[1]};
  clamp_slack(h, late ? &slack : nullptr, who.c_str());
  check_range(obstacles, (size_t)D.P * D.n_obs * 7, "obstacles");
  check_range(&obstacle_margin, 1, "obstacle_margin");
  check_range(&pair_margin, 1, "pair_margin");
  check_range(&separation, 1, "separation");
  if (tracks && sb.track_cost) check_range(sb.track_cost, (size_t)sb.n_tracks, "track_cost");
  if (tracked) check_tracked_first(h, *tracked);
  h->use_device();
  require_drained(h, who.c_str());
  sync(h);   // behind the running rollout, like the getters of its results
  select_scratch(h);
  // 1. the obstacle side of every population, as pmaf_select_clear runs it
  // (the tracked call: the columns of either list that ride on the OTHER member of the pair are the pair side's)
  const AuditColumns ride{pop_a, sb.pop_b, tracked ? attached_columns(h, pop_a, sb.pop_b) : 0,
                          tracked ? attached_columns(h, sb.pop_b, pop_a) : 0};
  const bool attached = (ride.cols_a | ride.cols_b) != 0;
  const SelectArgs S = select_obstacle_side(h, obstacles, obstacle_margin, horizon, skip_trailing != 0, tracked, &ride);
  XAuditWindow win{S.horizon};
  const XAuditAttach att{pop_a, sb.pop_b, h->d_sel_obs, false};
  // 2., 3. the windowed lengths and the cross audit on them; the matrix stays in the scratch
  const bool want = out.pair_steps != nullptr;
  int32_t keep = 0;   // (cross_audit_tracks takes "this step matrix is wanted" as a pointer)
  const XAuditBuf B = tracks ? cross_audit_tracks(h, pop_a, sb.n_tracks, sb.tracks, sb.n_track_points, separation,
                                                  late ? &slack : nullptr, nullptr, want ? &keep : nullptr,
                                                  want ? &keep : nullptr, who.c_str(), &win, sb.track_cost)
                             : cross_audit_populations(h, pop_a, sb.pop_b, separation, late ? &slack : nullptr, want, want,
                                                       who.c_str(), &win, attached ? &att : nullptr);
  // 4., 5. the joint reduction, the rule, the record and the adopt stores
  const size_t rec_at = select_pairclear_rec(D);
  double *rec = h->sel.host() + rec_at;
  PairClearArgs A{};
  A.clearance = B.clearance;
  A.step_a = want ? B.step : nullptr;
  A.step_b = want && late ? B.step_b : nullptr;
  A.cost_a = D.costs + (size_t)pop_a * D.N;
  A.clr_a = h->d_sel_clr + (size_t)pop_a * D.N;
  A.fv_a = h->d_sel_fv + (size_t)pop_a * D.N;
  if (tracks) {
    A.cost_b = sb.track_cost ? B.track_cost : nullptr;
  } else {
    A.cost_b = D.costs + (size_t)sb.pop_b * D.N;
    A.clr_b = h->d_sel_clr + (size_t)sb.pop_b * D.N;
    A.fv_b = h->d_sel_fv + (size_t)sb.pop_b * D.N;
  }
  A.len_a = B.win_a;
  A.len_b = B.win_b;
  A.n_a = D.N;
  A.n_b = n_b;
  A.pop_a = pop_a;
  A.pop_b = tracks ? -1 : sb.pop_b;
  A.obstacle_margin = obstacle_margin;
  A.pair_margin = pair_margin;
  A.prev_i = prev_pair ? prev_pair[0] : -1;
  A.prev_j = prev_pair ? prev_pair[1] : -1;
  A.adopt = adopt ? 1 : 0;
  A.partial = B.pc_partial;
  A.result = h->sel.dev() + rec_at;
  A.seq = (h->pairclear_seq += 1.0);
  pmaf_k_launch_pairclear(D, A, h->stream);
  HIP_CHECK(hipGetLastError());
  wait_select(h, rec, 1, PMAF_PAIRCLEAR_REC, A.seq, who.c_str());
  out.pair[0] = (int32_t)rec[0];
  out.pair[1] = (int32_t)rec[1];
  if (adopt && out.pair[0] >= 0 && (pop_a == 0 || sb.pop_b == 0)) h->has_best_h = 1;   // (has_best_h speaks for population 0)
  if (out.rule) *out.rule = (int32_t)rec[2];
  if (out.n_feasible) *out.n_feasible = (int32_t)rec[3];
  if (out.n_clear) { out.n_clear[0] = (int32_t)rec[4]; out.n_clear[1] = (int32_t)rec[5]; }
  if (out.pair_cost) *out.pair_cost = rec[6];
  if (out.pair_clearance) *out.pair_clearance = rec[7];
  if (out.obstacle_clearance) { out.obstacle_clearance[0] = rec[8]; out.obstacle_clearance[1] = rec[9]; }
  if (out.first_violation) { out.first_violation[0] = (int32_t)rec[10]; out.first_violation[1] = (int32_t)rec[11]; }
  if (out.worst_excess) *out.worst_excess = rec[12];
  if (out.pair_steps) { out.pair_steps[0] = (int32_t)rec[13]; out.pair_steps[1] = (int32_t)rec[14]; }
}

int pmaf_select_pair_clear(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles, double obstacle_margin,
                           int32_t horizon, int32_t skip_trailing, double separation, double pair_margin, const int32_t *late,
                           const int32_t *prev_pair, int32_t adopt, int32_t *pair, int32_t *rule, int32_t *n_feasible,
                           int32_t *n_clear, double *pair_cost, double *pair_clearance, double *obstacle_clearance,
                           int32_t *first_violation, double *worst_excess, int32_t *pair_steps) {
  return guarded([&] {
    REQUIRE(h && obstacles && pair, "pmaf_select_pair_clear: NULL argument");
    REQUIRE(pop_b >= 0, "pmaf_select_pair_clear: need two different populations of the handle");
    select_pair_clear(h, pop_a, PairClearSideB{pop_b, 0, nullptr, nullptr, nullptr}, obstacles, obstacle_margin, horizon,
                      skip_trailing, separation, pair_margin, late, prev_pair, adopt,
                      PairClearOut{pair, rule, n_feasible, n_clear, pair_cost, pair_clearance, obstacle_clearance,
                                   first_violation, worst_excess, pair_steps},
                      "pmaf_select_pair_clear");
  });
}

int pmaf_select_pair_clear_tracked(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles, const int32_t *first,
                                   double obstacle_margin, int32_t horizon, int32_t skip_trailing, double separation,
                                   double pair_margin, const int32_t *prev_pair, int32_t adopt, int32_t *pair, int32_t *rule,
                                   int32_t *n_feasible, int32_t *n_clear, double *pair_cost, double *pair_clearance,
                                   double *obstacle_clearance, int32_t *first_violation, double *worst_excess,
                                   int32_t *pair_steps) {
  return guarded([&] {
    REQUIRE(h && obstacles && pair, "pmaf_select_pair_clear_tracked: NULL argument");
    REQUIRE(pop_b >= 0, "pmaf_select_pair_clear_tracked: need two different populations of the handle");
    const TrackedCall T{first, "pmaf_select_pair_clear_tracked"};
    select_pair_clear(h, pop_a, PairClearSideB{pop_b, 0, nullptr, nullptr, nullptr}, obstacles, obstacle_margin, horizon,
                      skip_trailing, separation, pair_margin, nullptr, prev_pair, adopt,
                      PairClearOut{pair, rule, n_feasible, n_clear, pair_cost, pair_clearance, obstacle_clearance,
                                   first_violation, worst_excess, pair_steps},
                      T.who, &T);
  });
}

int pmaf_select_pair_clear_tracked_slack(pmaf_planner *h, int32_t pop_a, int32_t pop_b, const double *obstacles,
                                         const int32_t *first, double obstacle_margin, int32_t horizon, int32_t skip_trailing,
                                         double separation, double pair_margin, const int32_t *late, const int32_t *prev_pair,
                                         int32_t adopt, int32_t *pair, int32_t *rule, int32_t *n_feasible, int32_t *n_clear,
                                         double *pair_cost, double *pair_clearance, double *obstacle_clearance,
                                         int32_t *first_violation, double *worst_excess, int32_t *pair_steps) {
  return guarded([&] {
    REQUIRE(h && obstacles && pair, "pmaf_select_pair_clear_tracked_slack: NULL argument");
    REQUIRE(pop_b >= 0, "pmaf_select_pair_clear_tracked_slack: need two different populations of the handle");
    const TrackedCall T{first, "pmaf_select_pair_clear_tracked_slack"};
    select_pair_clear(h, pop_a, PairClearSideB{pop_b, 0, nullptr, nullptr, nullptr}, obstacles, obstacle_margin, horizon,
                      skip_trailing, separation, pair_margin, late, prev_pair, adopt,
                      PairClearOut{pair, rule, n_feasible, n_clear, pair_cost, pair_clearance, obstacle_clearance,
                                   first_violation, worst_excess, pair_steps},
                      T.who, &T);
  });
}

int pmaf_select_clear_tracks(pmaf_planner *h, int32_t pop, const double *obstacles, double obstacle_margin, int32_t horizon,
                             int32_t skip_trailing, int32_t n_tracks, const double *tracks, const int32_t *n_track_points,
                             const double *track_cost, double separation, double pair_margin, const int32_t *late,
                             const int32_t *prev_pair, int32_t adopt, int32_t *pair, int32_t *rule, int32_t *n_feasible,
                             int32_t *n_clear, double *pair_cost, double *pair_clearance, double *obstacle_clearance,
                             int32_t *first_violation, double *worst_excess, int32_t *pair_steps) {
  return guarded([&] {
    REQUIRE(h && obstacles && tracks && n_track_points && pair, "pmaf_select_clear_tracks: NULL argument");
    select_pair_clear(h, pop, PairClearSideB{-1, n_tracks, tracks, n_track_points, track_cost}, obstacles, obstacle_margin,
                      horizon, skip_trailing, separation, pair_margin, late, prev_pair, adopt,
                      PairClearOut{pair, rule, n_feasible, n_clear, pair_cost, pair_clearance, obstacle_clearance,
                                   first_violation, worst_excess, pair_steps},
                      "pmaf_select_clear_tracks");
  });
}

int pmaf_link_force(pmaf_planner *h, int32_t pop, int32_t n, const double *link_pos, const double *k_r_force,
                    const double *obstacles, double *out) {
  return guarded([&] {
    REQUIRE(h && link_pos && k_r_force && obstacles && out, "pmaf_link_force: NULL argument");
    REQUIRE(pop >= 0 && pop < h->D.P && n >= 0, "pmaf_link_force: bad population or count");
    if (n == 0) return;
    const double *sent = obstacles + ((size_t)pop * h->D.n_obs + (h->D.n_obs - 1)) * 7;
    check_range(link_pos, (size_t)n * 3, "pmaf_link_force: link_pos");
    check_range(k_r_force, (size_t)n, "pmaf_link_force: k_r_force");
    check_range(sent, 7, "pmaf_link_force: obstacles (last)");
    h->use_device();
    // per-handle scratch, grown on demand: [3n] link points | [n] gains | [7] obstacle | [3n] forces
    const size_t need = (size_t)n * 7 + 7;
    // (the smaller half decides: a half whose allocation failed holds nothing, and the next call grows both again)
    if (sizeof(double) * need > std::min(h->d_link.bytes(), h->h_link.bytes())) {
      sync(h);
      const size_t cap_d = need < 512 ? 512 : need * 2;
      h->d_link.reserve(sizeof(double) * cap_d);
      h->h_link.reserve(sizeof(double) * cap_d);
    }
    double *hb = h->h_link.get(), *db = h->d_link.get();
    std::memcpy(hb, link_pos, sizeof(double) * 3 * n);
    std::memcpy(hb + 3 * (size_t)n, k_r_force, sizeof(double) * n);
    std::memcpy(hb + 4 * (size_t)n, sent, sizeof(double) * 7);
    const size_t in_d = 4 * (size_t)n + 7;
    HIP_CHECK(hipMemcpyAsync(db, hb, sizeof(double) * in_d, hipMemcpyHostToDevice, h->stream));
    pmaf_k_launch_link_force(n, db, db + 3 * (size_t)n, db + 4 * (size_t)n, h->D.C.rad, h->D.C.shell, db + in_d, h->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hb + in_d, db + in_d, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, h->stream));
    sync(h);
    std::memcpy(out, hb + in_d, sizeof(double) * 3 * n);
  });
}

}  // extern "C"
