// pmaf_host_impl.hpp -- what the host units of libpmaf_hip.so share (pmaf_host.cpp, pmaf_host_audit.cpp,
// pmaf_host_exchange.cpp, pmaf_host_state.cpp; g++, plain C++ against the HIP runtime API): the handle, the error
// types behind every export's `guarded`, the owners of its scratch and pinned memory, the one bounded wait, and the few
// helpers one unit defines and another calls (namespace pmaf_host). No kernel unit includes it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

#include "../../include/pmaf.h"
#include "pmaf_comm.hpp"
#include "pmaf_types.hpp"
#include "pmaf_lpa_model.hpp"
#include "pmaf_route.hpp"
#include "pmaf_track.hpp"
#include "pmaf_ftrack.hpp"
#include "pmaf_fcouple.hpp"
#include "pmaf_ftingest.hpp"

using namespace pmaf;

struct HipError {
  hipError_t e;
  const char *what;
  const char *file;   // the unit (or this header) that threw
  int line;
};
#define HIP_CHECK(x)                                   \
  do {                                                 \
    hipError_t _e = (x);                               \
    if (_e != hipSuccess) throw HipError{_e, #x, __FILE__, __LINE__}; \
  } while (0)

struct StatusError {
  int code;
  std::string msg;
};
static void fail(int code, const std::string &msg) { throw StatusError{code, msg}; }

// Supported numeric range of every input (metres, m/s, gains, seconds): finite
// and either exactly 0 or 2^-100 <= |x| <= 2^100. Keeps all divisions / square
// roots of the path inside the exponent range where the hand-expanded
// sequences (MATH_XACT) equal the IEEE ones.
static void check_range(const double *v, size_t n, const char *what) {
  for (size_t i = 0; i < n; i++) {
    const double a = std::fabs(v[i]);
    if (!(a == 0.0 || (a >= 0x1p-100 && a <= 0x1p100)))
      fail(PMAF_ERR_INVALID, std::string(what) + ": value outside the supported numeric range (finite, 0 or 2^-100 <= |x| <= 2^100)");
  }
}

// ---- owners: what the handle allocates outside its checkpointed buffers is freed by `delete h` ----
// Grow-only buffer in device memory (DeviceBuf) or plain pinned host memory (PinnedBuf). reserve() is a no-op while the
// buffer is large enough; otherwise it frees, forgets the size, allocates, and records the size only after success --
// so a failed allocation leaves an empty buffer that the next call grows again. How many bytes a call needs, and what
// has to be drained before the old buffer may go, stays with the call.
template <typename T, bool PINNED>
class GrowBuf {
  T *p_ = nullptr;
  size_t bytes_ = 0;

 public:
  GrowBuf() = default;
  GrowBuf(const GrowBuf &) = delete;
  GrowBuf &operator=(const GrowBuf &) = delete;
  ~GrowBuf() { release(); }
  T *get() const { return p_; }
  size_t bytes() const { return bytes_; }
  void release() {
    if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    bytes_ = 0;
  }
  bool reserve(size_t bytes) {   // true: allocated anew (the old contents are gone)
    if (p_ && bytes <= bytes_) return false;
    release();
    HIP_CHECK(PINNED ? hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault) : hipMalloc((void **)&p_, bytes));
    bytes_ = bytes;
    return true;
  }
  void swap(GrowBuf &o) {   // (a buffer that grows and keeps its contents: filled beside the old one, then exchanged)
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
  }
};
template <typename T> using DeviceBuf = GrowBuf<T, false>;
template <typename T> using PinnedBuf = GrowBuf<T, true>;

// Mapped pinned pair: one allocation, the host pointer and its device alias, zero-filled.
class MappedBuf {
  double *h_ = nullptr, *d_ = nullptr;

 public:
  MappedBuf() = default;
  MappedBuf(const MappedBuf &) = delete;
  MappedBuf &operator=(const MappedBuf &) = delete;
  ~MappedBuf() { release(); }
  double *host() const { return h_; }
  double *dev() const { return d_; }
  void release() {
    if (h_) (void)hipHostFree(h_);
    h_ = d_ = nullptr;
  }
  void alloc(size_t bytes) {
    release();
    HIP_CHECK(hipHostMalloc((void **)&h_, bytes, hipHostMallocMapped));
    const hipError_t e = hipHostGetDevicePointer((void **)&d_, h_, 0);
    if (e != hipSuccess) release();   // never half a pair: host() != nullptr is what "allocated" means to the callers
    if (e != hipSuccess) throw HipError{e, "hipHostGetDevicePointer (mapped pair)", __FILE__, __LINE__};
    std::memset(h_, 0, bytes);
  }
};

struct pmaf_planner {
  DevView D{};
  int device = 0;
  // which rollout kernel this handle launches and with what (pmaf_route.hpp): everything the choice depends on, and the
  // choice -- recomputed by reroute() where an input changes, read everywhere else
  pmaf_route::Input route_in;
  pmaf_route::Route route;
  bool blocking_wait = false;  // PMAF_FLAG_BLOCKING_WAIT: pmaf_tick sleeps on an event instead of spinning on the mailbox
  size_t lds_manager = 0;
  hipModule_t ext_mod = nullptr;       // pmaf_debug_external_rollout: a rollout kernel loaded from a code object file
  hipFunction_t ext_fn = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev_mgr = nullptr;
  uint64_t mailbox_seq = 0;     // sequence number of the last pmaf_tick (mailbox entry 11)
  double tick_timeout_s = 5.0;  // PMAF_TICK_TIMEOUT_S: bound of pmaf_tick's wait for the manager kernel's result
  bool dbg_withhold = false;    // pmaf_debug_withhold_mailbox: the sequence number is not published (fault injection)
  // winner path in mapped pinned memory (pmaf_enable_winner_path): [P][cap][3] + header [P][4] = n_points, agent, 0, seq
  MappedBuf wp, wph;
  std::vector<int32_t> wp_np, wp_agent;
  double wp_seq = 0.0;          // sequence number the last selection published its path under (0: none yet)
  std::chrono::steady_clock::time_point last_tick_entry{};
  bool wp_timed = true;         // the last pmaf_tick's path latency has been booked (or there was no tick)
  std::vector<double> wp_us;
  // DevView::closest_idx: k_manager recomputes the table at the next reset when the caller has handed over a live
  // obstacle list that DIFFERS (bit for bit) from the previous one -- a node that passes the same static list every tick
  // pays for the table once
  bool closest_dirty = true;
  std::vector<double> last_live;   // the caller's last list, as given ([P][n_obs][7])
  // the COMPLETE list D.obs_live currently holds, as the caller gave it (empty: unknown): pmaf_tick does not hand a list
  // over again that is already resident -- the reference's node passes its obstacles_ with every call, and reading
  // 1.8 KB of mapped host memory in the manager kernel costs ~5 us of set-point latency (tools/ticklat.py)
  std::vector<double> live_resident;
  // (only the FIELD obstacles count -- the first n_obs - 1 rows of every population: the trailing repulsive obstacle,
  // which a host-coupled dual-arm run rewrites every tick, is not in the table)
  void note_live_obstacles(const double *obstacles) {
    const size_t row = (size_t)D.n_obs * 7, field = (size_t)(D.n_obs - 1) * 7;
    bool same = last_live.size() == (size_t)D.P * field;
    for (int p = 0; p < D.P && same; p++)
      same = std::memcmp(last_live.data() + p * field, obstacles + p * row, sizeof(double) * field) == 0;
    if (same) return;
    last_live.resize((size_t)D.P * field);
    for (int p = 0; p < D.P; p++) std::memcpy(last_live.data() + p * field, obstacles + p * row, sizeof(double) * field);
    closest_dirty = true;
  }
  // host-side clock of the last pmaf_tick calls (pmaf_get_tick_times_us): entry -> both launches enqueued, entry ->
  // set-point on the host; a ring of the newest TICK_RING calls
  static constexpr size_t TICK_RING = 8192;
  std::vector<float> tick_enq_us, tick_sp_us;
  size_t tick_head = 0, tick_count = 0;
  std::vector<void *> allocs;
  std::vector<size_t> alloc_bytes;  // size of every device buffer (state save / load)
  MappedBuf mbox;               // pinned [P][PMAF_MBOX] mailbox written by k_manager (through its device alias)
  // host copy of the real agent's state (getNextPosition / getNextVelocity /
  // getEEForce / getDistFromGoal must not wait for the running rollout)
  std::vector<double> real_pos_h, real_vel_h, real_force_h;
  MappedBuf zc;                 // mapped pinned obstacle buffer read by k_manager in pmaf_tick
  // closed loop: pmaf_set_real_position leaves the measured position [P][3] in mapped pinned memory and the NEXT manager
  // launch reads it from there (ManagerArgs::real_pos_src) -- the call neither waits for the running rollout nor puts a
  // copy command in front of the tick. One buffer is enough: every entry point that launches the manager kernel returns
  // only after that kernel has read its inputs.
  MappedBuf rp;
  bool real_pos_pending = false;
  // pop 0's D.has_best as the host knows it (pmaf_move_real's precondition without a device round trip): 1 after any
  // completed selection, 0 on a fresh handle, -1 unknown (after pmaf_load_state / pmaf_set_best with id 0: read back once)
  int has_best_h = 0;
  double call_seq = 0.0;        // mailbox sequence numbers of the manager launches that are not pmaf_ticks: -1, -2, ...
  // pmaf_tick gave up on its time limit with its launches still queued / running (they still read zc / rp and write
  // the mailbox): no further tick until the stream has been drained (pmaf_stop)
  bool tick_abandoned = false;
  // ---- winner-record exchange of sharded runs (pmaf_attach_comm) ----
  // Two exchange slots used alternately: the selection of tick k sends from slot k & 1, so its manager kernel only has
  // to wait for the exchange of tick k-2 (long through) -- never for the collective of the tick before, which a slower
  // peer rank may not even have joined yet.
  struct Exchange {
    pmaf_comm *c = nullptr;
    hipStream_t xp = nullptr;          // pack stream: k_winner_path (local work only, never behind a collective)
    hipStream_t xs = nullptr;          // exchange stream: all-gather + copy of the table to the host
    struct Slot {
      hipEvent_t ev_pack = nullptr;    // k_winner_path has read the scored paths
      hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;  // around ncclAllGather (timing)
      hipEvent_t ev_done = nullptr;    // table on the host
      double *d_send = nullptr, *d_recv = nullptr;  // [P][rec], [world][P][rec]
      double *h_send = nullptr, *h_recv = nullptr;  // pinned
      bool inflight = false;
      bool pack_pending = false;       // ev_pack recorded and not yet known to have completed
    } slot[2];
    int cur = 1;                       // slot of the last exchange begun (the next one takes cur ^ 1)
    double *paths_a = nullptr, *paths_b = nullptr;  // the two path buffers (a = the handle's original one)
    bool failed = false;               // the last exchange did not complete: pmaf_winners_wait reports it
    std::vector<double> ag_us;
    bool any_inflight() const { return slot[0].inflight || slot[1].inflight; }
  } x;
  // ---- peer mailboxes (pmaf_peer_*): header-only exchange without a collective ----
  struct Peer {
    bool on = false;
    int world = 0, rank = 0;
    double *inbox = nullptr;             // this rank's inbox [2][world][P][PMAF_PEER_SLOT] (device memory)
    bool inbox_fine = false;
    std::vector<double *> mapped;        // every rank's inbox as mapped into this process
    std::vector<char> opened;            // 1: mapped[r] came from hipIpcOpenMemHandle
    PeerView *d_view = nullptr;
    int32_t *d_couple = nullptr;
    double *d_radius = nullptr;
    std::vector<int32_t> couple_h;
    std::vector<double> radius_h;
    uint64_t tick = 0;                   // pmaf_ticks since pmaf_peer_connect = sequence number last published
    double us_per_tick = 0.01;           // wall_clock64 period
    std::vector<double> wait_us, pub_us;
  } peer;
  DeviceBuf<double> d_send1;           // send buffer of the one-shot pmaf_allgather_winners
  // host mirror of the predicted paths (pmaf_get_paths): the reference's node calls getPredictedPaths() /
  // getNumPredictionSteps(i) 3 x N times per tick (B/src/panda_bimanual_control.cpp:341-344) -- one D2H per
  // rollout generation serves them all
  uint64_t paths_gen = 1, mirror_gen = 0;   // bumped by everything that changes paths / n_points
  PinnedBuf<double> h_paths;                // pinned [P][N][cap][3], tails zeroed
  PinnedBuf<int32_t> h_np;                  // pinned [P][N]
  double *d_plan_obs = nullptr;        // [P][7][n_obs] the stepping API's obstacle list (pmaf_move_agents ...)
  double *d_plan_out = nullptr;        // [P][N] pmaf_eval_obstacle_distance
  int32_t *d_plan_calls = nullptr;     // [P]
  bool stepped = false;                // agents were moved / set by the stepping API: a rollout needs a reset first
  double exchange_timeout_s = 60.0;    // PMAF_EXCHANGE_TIMEOUT_S: bound of the wait for a winner exchange
  DeviceBuf<double> d_link;  // pmaf_link_force scratch, grown on demand: the device half ...
  PinnedBuf<double> h_link;  // ... and its pinned host half, the same size
  // pmaf_evaluate_paths / pmaf_evaluate_path scratch, grown on demand: the obstacle track [P][cap][3][n_obs] and the
  // outputs on the device, the outputs' pinned host mirror (one device-to-host copy per call)
  DeviceBuf<char> d_audit;
  PinnedBuf<char> h_audit;
  // pmaf_cross_audit / pmaf_cross_audit_tracks / pmaf_select_pair scratch, grown on demand: the clearance matrix and the
  // step matrix, the pair reduction's partials and result, the caller's tracks and their lengths
  DeviceBuf<char> d_xaudit;
  // pmaf_evaluate_paths_slack scratch, grown on demand: the five per-agent outputs on the device and their pinned host
  // mirror (pmaf_select_clear_slack needs neither: its audit writes the selection's d_sel_clr / d_sel_fv)
  DeviceBuf<char> d_oslack;
  PinnedBuf<char> h_oslack;
  // pmaf_select_clear / pmaf_adopt_best scratch, allocated by the first call; none of it is planner state. Mapped pinned
  // host memory of the call's own (`sel`, NOT `zc`: the list must not become the resident live list): the list [P][7][n_obs] |
  // the result records [P][PMAF_SELECT_REC] | the previous picks [P] int32. On the device: the staged list, the audit's
  // per-agent clearance and first violation, pmaf_adopt_best's indices for handles of many populations.
  MappedBuf sel;
  double *d_sel_obs = nullptr, *d_sel_clr = nullptr;
  int32_t *d_sel_fv = nullptr, *d_adopt_idx = nullptr;
  double sel_seq = 0.0;         // sequence number of the last pmaf_select_clear (result record entry 7)
  double pairclear_seq = 0.0;   // ... of the last joint selection (its record's last entry)
  // ---- repulsive track (include/pmaf.h "repulsive track"): inputs, not planner state -- none of it is in the checkpoint blob.
  // The device buffer [P][stride][3] + lengths [P] (grow-only) holds what the next rollout launch follows: the caller's
  // upload, overwritten for coupled populations by k_track_from_best in front of every launch. The host keeps the upload
  // ([P][up_max][3], up_len) so that uncoupling or a grown buffer can put it back.
  struct Track {
    DeviceBuf<double> d_pts;
    DeviceBuf<int32_t> d_len, d_src;              // d_src: [P] source population of the coupling (-1: none)
    int stride = 0;                               // points per population the device buffer holds
    std::vector<double> up;
    std::vector<int32_t> up_len;
    int up_max = 0;
    bool uploaded = false;                        // some up_len > 0
    bool coupled = false;
    // the coupled tracks were taken in front of a reset that rewrites the paths (pmaf_reset_agents of the five-call tick):
    // the next rollout launch follows them instead of copying again
    bool captured = false;
    std::vector<int32_t> src;
    int shift = 0;
    bool on() const { return uploaded || coupled; }
  } trk;
  // ---- obstacle tracks (include/pmaf.h "obstacle tracks"): inputs like the repulsive track, not in the checkpoint blob.
  // d_pts [P][stride][6][64] (pmaf_ftrack.hpp; grow-only), d_len / d_first [P]: what the next rollout launch follows. The
  // host keeps the lengths and offsets (the refusals and the detach need them), never the points. d_no_pts / d_no_len: the
  // one-point, zero-length repulsive track k_rollout_w64_ftrack is handed while the handle has no repulsive track.
  struct FieldTrack {
    DeviceBuf<double> d_pts, d_no_pts;
    DeviceBuf<int32_t> d_len, d_first, d_no_len;
    int stride = 0;                               // points per population the device buffer holds (>= 1 once allocated)
    std::vector<int32_t> len, first;
    bool attached = false;                        // some len > 0
    // the device-side source (pmaf_couple_obstacle_tracks, pmaf_fcouple.hpp): field obstacles that ride on another
    // population's selected path. The coupled populations' points, len (cap or 0) and first (0) are written on the
    // device -- k_fcouple_take at the capture moment of the repulsive coupling, k_fcouple_compose in front of every
    // rollout launch --; the host's len / first of such a population stay 0. stride >= cap while coupled.
    bool coupled = false;
    bool captured = false;                        // as Track::captured: the selected paths were taken in front of a reset
    std::vector<int32_t> src;                     // [P][M], -1: not attached
    std::vector<char> pop_coupled;                // [P]: some column of the population is attached
    int shift = 0;
    DeviceBuf<int32_t> d_src, d_is_src, d_sel_n;  // [P][64], [P], [P]
    DeviceBuf<double> d_scale, d_anchor, d_sel_pts;   // [P][64], [P][3][64], [P][cap][3]
    // the device-memory source (pmaf_set_obstacle_tracks_device, pmaf_ftingest.hpp): the call's lengths as its kernels
    // read them and the verdict word of its range check; scratch of the call, nothing the rollouts read
    DeviceBuf<int32_t> d_in_len;                  // [P]
    DeviceBuf<unsigned long long> d_verdict;      // one word
    bool is_coupled(int p) const { return coupled && pop_coupled[(size_t)p] != 0; }
    bool on() const { return attached || coupled; }
  } ftrk;
  double *d_reset_in = nullptr; // [P][6]
  int32_t *d_agent_id = nullptr;// [P]
  CostParams cp{};
  bool cp_valid = false;        // cp holds the workspace terms the stored cost_ws was computed with
  bool scores_valid = false;
  bool rollout_pending = false; // agents were (re)set since the last rollout
  std::vector<std::vector<double>> real_path;  // per population, xyz triples
  std::vector<double> goal_h;
  // profiling
  bool profiling = false;
  int prof_every = 1;           // event timing on every prof_every-th rollout launch (pmaf_set_profiling's argument)
  int64_t prof_phase = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_free, ev_inflight;
  double rollout_ms = 0.0, last_rollout_ms = 0.0;
  int64_t launches = 0, timed_launches = 0;

  template <typename T>
  T *dalloc(size_t n) {
    void *p = nullptr;
    HIP_CHECK(hipMalloc(&p, sizeof(T) * (n ? n : 1)));
    allocs.push_back(p);
    alloc_bytes.push_back(sizeof(T) * (n ? n : 1));
    HIP_CHECK(hipMemsetAsync(p, 0, sizeof(T) * (n ? n : 1), stream));
    return static_cast<T *>(p);
  }
  // scratch that is not planner state (not in the checkpoint blob); freed with the handle
  std::vector<void *> scratch;
  template <typename T>
  T *dalloc_untracked(size_t n) {
    void *p = nullptr;
    HIP_CHECK(hipMalloc(&p, sizeof(T) * (n ? n : 1)));
    scratch.push_back(p);
    return static_cast<T *>(p);
  }
  template <typename T>
  void upload(T *dst, const T *src, size_t n) {
    HIP_CHECK(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  template <typename T>
  void download(T *dst, const T *src, size_t n) {
    HIP_CHECK(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  void use_device() { HIP_CHECK(hipSetDevice(device)); }
};

void pmaf_set_last_error(const std::string &msg);   // pmaf_host.cpp: the thread-local message of pmaf_last_error

template <typename F>
static int guarded(F &&f) {
  try {
    f();
    return PMAF_OK;
  } catch (const StatusError &e) {
    pmaf_set_last_error(e.msg);
    return e.code;
  } catch (const HipError &e) {
    char buf[512];
    snprintf(buf, sizeof(buf), "HIP error %d (%s) at %s [%s:%d]", (int)e.e, hipGetErrorString(e.e), e.what, e.file, e.line);
    pmaf_set_last_error(buf);
    return PMAF_ERR_DEVICE;
  } catch (const std::bad_alloc &) {
    pmaf_set_last_error("host allocation failed");
    return PMAF_ERR_NOMEM;
  } catch (...) {
    pmaf_set_last_error("unknown error");
    return PMAF_ERR_INVALID;
  }
}

#define REQUIRE(c, msg) do { if (!(c)) fail(PMAF_ERR_INVALID, msg); } while (0)

// one spin of a polling loop; the weight it returns is what bounded_wait counts it as
static inline unsigned spin_pause() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
  return 1;
}

// The one bounded wait of the host side: spin until done() holds -- a word in host-visible memory, an event -- but never
// for ever. pause() passes the time between two looks and returns the spins it counts as; every `period` spins (a power
// of two) the wall clock is read -- started lazily, at the first such poll -- and query() asks whether the work is still
// running (hipStreamQuery / hipEventQuery: hipErrorNotReady = yes), so that a failed or finished launch cannot leave the
// host spinning: an error is thrown, and work that is through without done() fails with `who` + `unpublished`. Past
// `limit_s` seconds expired() marks the handle (its kernels are still queued or running) and throws what the call reports.
template <typename Done, typename Query, typename Pause, typename Expired>
static void bounded_wait(Done done, Query query, Pause pause, unsigned period, double limit_s, Expired expired,
                         const char *who, const char *unpublished) {
  std::chrono::steady_clock::time_point t_start{};
  bool timing = false;
  unsigned spins = 0;
  while (!done()) {
    const unsigned w = pause();
    if (((spins += w) & (period - 1)) >= w) continue;
    const auto now = std::chrono::steady_clock::now();
    if (!timing) { timing = true; t_start = now; }
    else if (std::chrono::duration<double>(now - t_start).count() > limit_s) expired();
    const hipError_t e = query();
    if (e == hipErrorNotReady) continue;
    if (e != hipSuccess) throw HipError{e, "hipStreamQuery (bounded wait)", __FILE__, __LINE__};
    if (!done()) fail(PMAF_ERR_DEVICE, std::string(who) + unpublished);
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}
// done() of a wait for `count` words in host-visible memory, `stride` doubles apart, each of which a kernel sets to `seq`
// (the mailbox's sequence numbers, a selection's records, the winner path's headers): looked at in turn
struct SeqWords {
  const volatile double *word;
  int count;
  size_t stride;
  double seq;
  int at = 0;
  bool operator()() {
    while (at < count && word[at * stride] == seq) at++;
    return at == count;
  }
};

// ---- defined in one host unit, called from another (not exported: the library's symbols stay those of include/pmaf.h) ----
namespace pmaf_host __attribute__((visibility("hidden"))) {
inline size_t winner_rec(const pmaf_planner *h) { return PMAF_WINNER_HDR + (size_t)h->D.cap * 3; }
// pmaf_host.cpp
void sync(pmaf_planner *h);
void require_drained(pmaf_planner *h, const char *who);
void aos_to_soa(const double *aos, double *soa, int P, int n_obs);
const double *upload_plan_obstacles(pmaf_planner *h, const double *obstacles);
void flush_real_position(pmaf_planner *h);
void refresh_plain_step(pmaf_planner *h, const double *k_attr);
// pmaf_host_exchange.cpp
void finish_exchanges(pmaf_planner *h);
pmaf_planner::Exchange::Slot &claim_exchange_slot(pmaf_planner *h);
void begin_exchange(pmaf_planner *h, const double *scored_paths);
void detach_comm(pmaf_planner *h);
int peer_book_tick(pmaf_planner *h);
void peer_disconnect(pmaf_planner *h);
}  // namespace pmaf_host
using namespace pmaf_host;
