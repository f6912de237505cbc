// pmaf_host_state.cpp -- pmaf_state_size / pmaf_save_state / pmaf_load_state: the handle's checkpoint blob, i.e. the
// buffers of pmaf_planner::dalloc in the order pmaf_create made them plus the host-side planner state.
#include "pmaf_host_impl.hpp"

extern "C" {

// ---- checkpoint / resume ----------------------------------------------------
// The blob holds every device buffer of the handle (agents' rotation vectors,
// known flags, paths, real agent, best-agent copy, obstacle tables ...) plus
// the host-side planner state (real agent's trajectory, scoring parameters).
// the blob stores the handle's own buffers: with a communicator attached the current paths may live in the second
// path buffer -- finish the exchange in flight and move them back
static void normalise_path_buffer(pmaf_planner *h) {
  if (!h->x.c) return;
  finish_exchanges(h);
  if (h->D.paths != h->x.paths_a) {
    HIP_CHECK(hipMemcpy(h->x.paths_a, h->x.paths_b, sizeof(double) * (size_t)h->D.P * h->D.N * h->D.cap * 3, hipMemcpyDeviceToDevice));
    h->D.paths = h->x.paths_a;
  }
}

struct StateHeader {
  uint64_t magic;
  int32_t abi, P, N, n_obs, cap, n_bufs;
  int32_t cp_valid, scores_valid, rollout_pending, stepped;
  uint64_t dev_bytes;
};
static const uint64_t kStateMagic = 0x504d41465f535431ull;  // "PMAF_ST1"

static size_t state_bytes(const pmaf_planner *h) {
  size_t n = sizeof(StateHeader) + sizeof(CostParams) + sizeof(PopConst);
  for (size_t b : h->alloc_bytes) n += b;
  n += sizeof(double) * 9 * (size_t)h->D.P;                    // host mirror of the real agent
  for (auto &rp : h->real_path) n += sizeof(uint64_t) + sizeof(double) * rp.size();
  return n;
}

size_t pmaf_state_size(const pmaf_planner *h) { return h ? state_bytes(h) : 0; }

int pmaf_save_state(pmaf_planner *h, void *blob, size_t bytes) {
  return guarded([&] {
    REQUIRE(h && blob, "pmaf_save_state: NULL argument");
    REQUIRE(bytes >= state_bytes(h), "pmaf_save_state: buffer too small (see pmaf_state_size)");
    h->use_device();
    sync(h);
    normalise_path_buffer(h);
    flush_real_position(h);   // (closed loop: a measured position not yet consumed by a manager launch)
    char *w = static_cast<char *>(blob);
    StateHeader hd{};
    hd.magic = kStateMagic; hd.abi = PMAF_ABI_VERSION;
    hd.P = h->D.P; hd.N = h->D.N; hd.n_obs = h->D.n_obs; hd.cap = h->D.cap; hd.n_bufs = (int32_t)h->allocs.size();
    hd.cp_valid = h->cp_valid; hd.scores_valid = h->scores_valid; hd.rollout_pending = h->rollout_pending;
    hd.stepped = h->stepped;
    hd.dev_bytes = 0;
    for (size_t b : h->alloc_bytes) hd.dev_bytes += b;
    std::memcpy(w, &hd, sizeof(hd)); w += sizeof(hd);
    std::memcpy(w, &h->cp, sizeof(CostParams)); w += sizeof(CostParams);
    std::memcpy(w, &h->D.C, sizeof(PopConst)); w += sizeof(PopConst);
    for (size_t i = 0; i < h->allocs.size(); i++) {
      HIP_CHECK(hipMemcpyAsync(w, h->allocs[i], h->alloc_bytes[i], hipMemcpyDeviceToHost, h->stream));
      w += h->alloc_bytes[i];
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));
    const size_t n3 = sizeof(double) * 3 * (size_t)h->D.P;
    std::memcpy(w, h->real_pos_h.data(), n3); w += n3;
    std::memcpy(w, h->real_vel_h.data(), n3); w += n3;
    std::memcpy(w, h->real_force_h.data(), n3); w += n3;
    for (auto &rp : h->real_path) {
      uint64_t n = rp.size();
      std::memcpy(w, &n, sizeof(n)); w += sizeof(n);
      std::memcpy(w, rp.data(), sizeof(double) * n); w += sizeof(double) * n;
    }
  });
}

int pmaf_load_state(pmaf_planner *h, const void *blob, size_t bytes) {
  return guarded([&] {
    REQUIRE(h && blob, "pmaf_load_state: NULL argument");
    REQUIRE(bytes >= sizeof(StateHeader) + sizeof(CostParams) + sizeof(PopConst), "pmaf_load_state: blob too small");
    const char *r = static_cast<const char *>(blob);
    StateHeader hd;
    std::memcpy(&hd, r, sizeof(hd)); r += sizeof(hd);
    uint64_t dev = 0;
    for (size_t b : h->alloc_bytes) dev += b;
    REQUIRE(hd.magic == kStateMagic && hd.abi == PMAF_ABI_VERSION, "pmaf_load_state: not a pmaf state blob of this ABI version");
    REQUIRE(hd.P == h->D.P && hd.N == h->D.N && hd.n_obs == h->D.n_obs && hd.cap == h->D.cap &&
                hd.n_bufs == (int32_t)h->allocs.size() && hd.dev_bytes == dev,
            "pmaf_load_state: blob was saved from a handle with different dimensions");
    REQUIRE(bytes >= sizeof(StateHeader) + sizeof(CostParams) + sizeof(PopConst) + dev + sizeof(double) * 9 * (size_t)h->D.P,
            "pmaf_load_state: blob truncated");
    h->use_device();
    sync(h);
    normalise_path_buffer(h);
    std::memcpy(&h->cp, r, sizeof(CostParams)); r += sizeof(CostParams);
    std::memcpy(&h->D.C, r, sizeof(PopConst)); r += sizeof(PopConst);
    for (size_t i = 0; i < h->allocs.size(); i++) {
      HIP_CHECK(hipMemcpyAsync(h->allocs[i], r, h->alloc_bytes[i], hipMemcpyHostToDevice, h->stream));
      r += h->alloc_bytes[i];
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));
    refresh_plain_step(h, nullptr);                                 // the blob's gains and mass, not the handle's
    h->download(h->goal_h.data(), h->D.goal, (size_t)h->D.P * 3);  // host copy of the goals
    const size_t n3 = sizeof(double) * 3 * (size_t)h->D.P;
    std::memcpy(h->real_pos_h.data(), r, n3); r += n3;
    std::memcpy(h->real_vel_h.data(), r, n3); r += n3;
    std::memcpy(h->real_force_h.data(), r, n3); r += n3;
    const char *end = static_cast<const char *>(blob) + bytes;
    for (auto &rp : h->real_path) {
      uint64_t n = 0;
      REQUIRE(r + sizeof(n) <= end, "pmaf_load_state: blob truncated");
      std::memcpy(&n, r, sizeof(n)); r += sizeof(n);
      REQUIRE(r + sizeof(double) * n <= end, "pmaf_load_state: blob truncated");
      rp.assign(reinterpret_cast<const double *>(r), reinterpret_cast<const double *>(r) + n);
      r += sizeof(double) * n;
    }
    h->paths_gen++;
    h->cp_valid = hd.cp_valid != 0;
    h->scores_valid = hd.scores_valid != 0;
    h->rollout_pending = hd.rollout_pending != 0;
    h->stepped = hd.stepped != 0;
    h->real_pos_pending = false;
    h->has_best_h = -1;        // (the blob's: read back when pmaf_move_real asks)
    h->closest_dirty = true;   // (the blob's table matches its obs_start; recompute at the next reset all the same)
    h->last_live.clear();
    h->live_resident.clear();
  });
}

}  // extern "C"
