// pmaf_host_exchange.cpp -- what a handle shares with other ranks: the winner-record exchange of sharded runs
// (pmaf_attach_comm; the communicators themselves: pmaf_shard.cpp) and the peer mailboxes (pmaf_peer_*). pmaf_tick
// calls in here only with a communicator attached or peers connected.
#include "pmaf_host_impl.hpp"

// ---- winner-record exchange ---------------------------------------------------
// complete the exchange in flight (if any): RCCL -- wait for the table on the host and book the all-gather's device
// time; host transport -- wait for the packed records, then run the caller's collective here
static void finish_exchange(pmaf_planner *h, int which) {
  pmaf_planner::Exchange &x = h->x;
  pmaf_planner::Exchange::Slot &sl = x.slot[which];
  if (!sl.inflight) return;
  // Whatever happens below, this exchange is over: a failed one must not be retried by the next call (the ranks
  // would no longer issue their collectives in the same order)
  sl.inflight = false;
  // normally long through; poll instead of a blocking wait (whose wake-up latency would land on the next tick's
  // enqueue when the exchange is still in flight). Bounded: a peer that died leaves ncclAllGather waiting for ever --
  // after PMAF_EXCHANGE_TIMEOUT_S (default 60 s) the call fails with PMAF_ERR_DEVICE instead of spinning on
  // (here the look itself is the event query: what the poll asks is its last answer, and it yields the core first)
  hipError_t e = hipSuccess;
  bounded_wait([&] { return (e = hipEventQuery(sl.ev_done)) != hipErrorNotReady; },
               [&] { std::this_thread::yield(); return e; }, spin_pause, 1u << 20, h->exchange_timeout_s,
               [&] {
                 x.failed = true;
                 fail(PMAF_ERR_DEVICE, "winner exchange: the all-gather did not complete within the time limit (a peer rank "
                                       "gone? PMAF_EXCHANGE_TIMEOUT_S)");
               },
               "", "");
  if (e != hipSuccess) { x.failed = true; throw HipError{e, "hipEventQuery (winner exchange)", __FILE__, __LINE__}; }
  sl.pack_pending = false;
  const size_t n_local = (size_t)h->D.P * winner_rec(h);
  if (x.c->rccl) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, sl.ev_t0, sl.ev_t1));
    x.ag_us.push_back((double)ms * 1e3);
  } else {
    const auto t0 = std::chrono::steady_clock::now();
    if (x.c->fn(x.c->ctx, sl.h_send, sl.h_recv, n_local * sizeof(double)) != 0) {
      x.failed = true;
      fail(PMAF_ERR_DEVICE, "winner exchange: the host all-gather callback failed");
    }
    x.ag_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    HIP_CHECK(hipMemcpyAsync(sl.d_recv, sl.h_recv, n_local * x.c->world * sizeof(double), hipMemcpyHostToDevice, x.xs));
    HIP_CHECK(hipStreamSynchronize(x.xs));
  }
  if (x.ag_us.size() > (1u << 20)) x.ag_us.erase(x.ag_us.begin(), x.ag_us.begin() + (1u << 19));
}
// all exchanges in flight, oldest first (the host transport runs the callers' collectives here: same order on every rank)
void pmaf_host::finish_exchanges(pmaf_planner *h) {
  finish_exchange(h, h->x.cur ^ 1);
  finish_exchange(h, h->x.cur);
}
// the slot the next selection will send from: its previous exchange (two selections ago) must be through, and so
// must the pack kernel of the LAST exchange, which reads the path buffer the rollout launched next overwrites
// (local work on its own stream -- this wait never involves a peer)
pmaf_planner::Exchange::Slot &pmaf_host::claim_exchange_slot(pmaf_planner *h) {
  pmaf_planner::Exchange &x = h->x;
  finish_exchange(h, x.cur ^ 1);
  pmaf_planner::Exchange::Slot &last = x.slot[x.cur];
  if (last.pack_pending) {
    if (hipEventQuery(last.ev_pack) != hipSuccess) HIP_CHECK(hipEventSynchronize(last.ev_pack));
    last.pack_pending = false;
  }
  return x.slot[x.cur ^ 1];
}

// pack the selected agents' paths out of `scored_paths` behind the headers k_manager wrote into the claimed slot's
// send buffer and all-gather the records.
// Called once the HOST knows that k_manager has written the record headers (pmaf_tick: the mailbox's sequence number
// has arrived, and the headers are stored before it behind a system-scope fence; pmaf_evaluate: the stream is
// synchronised): the exchange streams then need no event from the handle's stream -- a cross-stream event between
// the manager and the rollout cost 4-7 us per tick (measured), this costs the rollout nothing.
void pmaf_host::begin_exchange(pmaf_planner *h, const double *scored_paths) {
  pmaf_planner::Exchange &x = h->x;
  x.cur ^= 1;
  pmaf_planner::Exchange::Slot &sl = x.slot[x.cur];
  const size_t n_local = (size_t)h->D.P * winner_rec(h);
  pmaf_k_launch_winner_path(h->D, scored_paths, sl.d_send, x.xp);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(sl.ev_pack, x.xp));
  sl.pack_pending = true;
  HIP_CHECK(hipStreamWaitEvent(x.xs, sl.ev_pack, 0));
  if (x.c->rccl) {
    HIP_CHECK(hipEventRecord(sl.ev_t0, x.xs));
    const std::string err = pmaf_comm_enqueue_allgather(x.c, sl.d_send, sl.d_recv, n_local, x.xs);
    if (!err.empty()) fail(PMAF_ERR_DEVICE, err);
    HIP_CHECK(hipEventRecord(sl.ev_t1, x.xs));
    HIP_CHECK(hipMemcpyAsync(sl.h_recv, sl.d_recv, n_local * x.c->world * sizeof(double), hipMemcpyDeviceToHost, x.xs));
  } else {
    HIP_CHECK(hipMemcpyAsync(sl.h_send, sl.d_send, n_local * sizeof(double), hipMemcpyDeviceToHost, x.xs));
  }
  HIP_CHECK(hipEventRecord(sl.ev_done, x.xs));
  sl.inflight = true;
  x.failed = false;
}

void pmaf_host::detach_comm(pmaf_planner *h) {
  pmaf_planner::Exchange &x = h->x;
  if (!x.c) return;
  h->paths_gen++;
  // an RCCL all-gather already enqueued completes (every rank enqueued it); a host collective not yet run is dropped
  if (x.xp) (void)hipStreamSynchronize(x.xp);
  if (x.any_inflight() && x.xs) (void)hipStreamSynchronize(x.xs);
  (void)hipStreamSynchronize(h->stream);
  if (h->D.paths != x.paths_a) {  // the handle goes back to its own path buffer
    (void)hipMemcpy(x.paths_a, x.paths_b, sizeof(double) * (size_t)h->D.P * h->D.N * h->D.cap * 3, hipMemcpyDeviceToDevice);
    h->D.paths = x.paths_a;
  }
  if (x.paths_b) (void)hipFree(x.paths_b);
  for (auto &sl : x.slot) {
    if (sl.d_send) (void)hipFree(sl.d_send);
    if (sl.d_recv) (void)hipFree(sl.d_recv);
    if (sl.h_send) (void)hipHostFree(sl.h_send);
    if (sl.h_recv) (void)hipHostFree(sl.h_recv);
    for (hipEvent_t e : {sl.ev_pack, sl.ev_t0, sl.ev_t1, sl.ev_done}) if (e) (void)hipEventDestroy(e);
  }
  if (x.xp) (void)hipStreamDestroy(x.xp);
  if (x.xs) (void)hipStreamDestroy(x.xs);
  x = pmaf_planner::Exchange{};
}

// ---- peer mailboxes ----------------------------------------------------------
struct PeerHandleBlob {   // what pmaf_peer_export hands out (PMAF_PEER_HANDLE_BYTES)
  uint64_t magic;
  int64_t pid;
  uint64_t ptr;           // the inbox in the exporting process (used when the importer IS that process)
  int32_t world, P, device, fine;   // fine: the inbox is fine-grained device memory
  hipIpcMemHandle_t ipc;
  int32_t pci[3];                   // PCI domain / bus / device of the exporting GPU (ordinals differ between processes)
  unsigned char fill[PMAF_PEER_HANDLE_BYTES - 40 - sizeof(hipIpcMemHandle_t) - 12];
};
static void pci_id_of(int device, int32_t out[3]) {
  int v = 0;
  out[0] = (hipDeviceGetAttribute(&v, hipDeviceAttributePciDomainID, device) == hipSuccess) ? v : -1;
  out[1] = (hipDeviceGetAttribute(&v, hipDeviceAttributePciBusId, device) == hipSuccess) ? v : -1;
  out[2] = (hipDeviceGetAttribute(&v, hipDeviceAttributePciDeviceId, device) == hipSuccess) ? v : -1;
  (void)hipGetLastError();
}
static_assert(sizeof(PeerHandleBlob) == PMAF_PEER_HANDLE_BYTES, "pmaf.h: PMAF_PEER_HANDLE_BYTES");
static const uint64_t kPeerMagic = 0x504d41465f505232ull;  // "PMAF_PR2" (the blob of ABI 5 changed layout: pad -> fine, pci[3])

static size_t peer_inbox_doubles(int world, int P) { return (size_t)2 * world * P * PMAF_PEER_SLOT; }

// after the mailbox of a tick has arrived: the wait for the coupled header / the publish time of this tick's manager
// kernel, and whether a header it waited for never came
// returns the worst peer status of the tick: 0 ok, 1 time-out, 2 the source ran ahead, 3 coupling not mutual
int pmaf_host::peer_book_tick(pmaf_planner *h) {
  pmaf_planner::Peer &pr = h->peer;
  double w = 0.0, pb = 0.0;
  int late = 0;
  for (int p = 0; p < h->D.P; p++) {
    const double *o = h->mbox.host() + p * PMAF_MBOX;
    w = std::max(w, o[12]);
    pb = std::max(pb, o[13]);
    late = std::max(late, (int)o[14]);
  }
  pr.wait_us.push_back(w * pr.us_per_tick);
  pr.pub_us.push_back(pb * pr.us_per_tick);
  if (pr.wait_us.size() > (1u << 20)) {
    pr.wait_us.erase(pr.wait_us.begin(), pr.wait_us.begin() + (1u << 19));
    pr.pub_us.erase(pr.pub_us.begin(), pr.pub_us.begin() + (1u << 19));
  }
  return late;
}

void pmaf_host::peer_disconnect(pmaf_planner *h) {
  pmaf_planner::Peer &pr = h->peer;
  h->live_resident.clear();   // (a coupled trailing obstacle was written on the device: the caller's list is handed over again)
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (size_t r = 0; r < pr.mapped.size(); r++)
    if (pr.opened[r] && pr.mapped[r]) (void)hipIpcCloseMemHandle(pr.mapped[r]);
  if (pr.d_view) (void)hipFree(pr.d_view);
  if (pr.d_couple) (void)hipFree(pr.d_couple);
  if (pr.d_radius) (void)hipFree(pr.d_radius);
  if (pr.inbox) (void)hipFree(pr.inbox);
  pr = pmaf_planner::Peer{};
}

extern "C" {

size_t pmaf_winner_record_doubles(const pmaf_planner *h) { return h ? winner_rec(h) : 0; }

int pmaf_write_winner_records(pmaf_planner *h, void *dst_device, size_t bytes) {
  return guarded([&] {
    REQUIRE(h && dst_device, "pmaf_write_winner_records: NULL argument");
    REQUIRE(bytes >= sizeof(double) * pmaf_winner_record_doubles(h) * h->D.P, "pmaf_write_winner_records: buffer too small");
    h->use_device();
    flush_real_position(h);
    pmaf_k_launch_winner(h->D, (double *)dst_device, h->stream);
    HIP_CHECK(hipGetLastError());
  });
}

int pmaf_allgather_winners(pmaf_planner *h, pmaf_comm *c, void *recv_device, size_t bytes) {
  return guarded([&] {
    REQUIRE(h && c && recv_device, "pmaf_allgather_winners: NULL argument");
    const size_t n_local = (size_t)h->D.P * winner_rec(h);
    REQUIRE(bytes >= sizeof(double) * n_local * (size_t)c->world, "pmaf_allgather_winners: receive buffer too small");
    h->use_device();
    h->d_send1.reserve(sizeof(double) * n_local);
    flush_real_position(h);
    pmaf_k_launch_winner(h->D, h->d_send1.get(), h->stream);
    HIP_CHECK(hipGetLastError());
    if (c->rccl) {
      // stream-ordered behind the pack kernel: no host synchronisation between the two
      const std::string err = pmaf_comm_enqueue_allgather(c, h->d_send1.get(), (double *)recv_device, n_local, h->stream);
      if (!err.empty()) fail(PMAF_ERR_DEVICE, err);
    } else {
      std::vector<double> snd(n_local), rcv(n_local * (size_t)c->world);
      h->download(snd.data(), h->d_send1.get(), n_local);
      if (c->fn(c->ctx, snd.data(), rcv.data(), n_local * sizeof(double)) != 0)
        fail(PMAF_ERR_DEVICE, "pmaf_allgather_winners: the host all-gather callback failed");
      h->upload((double *)recv_device, rcv.data(), rcv.size());
    }
  });
}

int pmaf_attach_comm(pmaf_planner *h, pmaf_comm *c) {
  return guarded([&] {
    REQUIRE(h, "pmaf_attach_comm: NULL handle");
    h->use_device();
    sync(h);
    detach_comm(h);
    if (!c) return;
    REQUIRE(!c->rccl || c->device == h->device, "pmaf_attach_comm: the communicator lives on another device than the handle");
    pmaf_planner::Exchange &x = h->x;
    const size_t n_local = (size_t)h->D.P * winner_rec(h);
    const size_t path_bytes = sizeof(double) * (size_t)h->D.P * h->D.N * h->D.cap * 3;
    try {
      {
        // high-priority streams: their own hardware queues, so the pack kernel and the all-gather are dispatched beside
        // the rollout instead of queueing with it (streams of equal priority may share a hardware queue: measured
        // +48 us per C2 tick with the exchange on a default-priority stream)
        int lo = 0, hi = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_CHECK(hipStreamCreateWithPriority(&x.xp, hipStreamNonBlocking, hi));
        HIP_CHECK(hipStreamCreateWithPriority(&x.xs, hipStreamNonBlocking, hi));
      }
      for (auto &sl : x.slot) {
        HIP_CHECK(hipEventCreateWithFlags(&sl.ev_pack, hipEventDisableTiming));
        HIP_CHECK(hipEventCreate(&sl.ev_t0));
        HIP_CHECK(hipEventCreate(&sl.ev_t1));
        HIP_CHECK(hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
        HIP_CHECK(hipMalloc((void **)&sl.d_send, sizeof(double) * n_local));
        HIP_CHECK(hipMalloc((void **)&sl.d_recv, sizeof(double) * n_local * (size_t)c->world));
        HIP_CHECK(hipHostMalloc((void **)&sl.h_send, sizeof(double) * n_local, hipHostMallocDefault));
        HIP_CHECK(hipHostMalloc((void **)&sl.h_recv, sizeof(double) * n_local * (size_t)c->world, hipHostMallocDefault));
        HIP_CHECK(hipMemset(sl.d_send, 0, sizeof(double) * n_local));
        HIP_CHECK(hipMemset(sl.d_recv, 0, sizeof(double) * n_local * (size_t)c->world));
        std::memset(sl.h_recv, 0, sizeof(double) * n_local * (size_t)c->world);
      }
      HIP_CHECK(hipMalloc((void **)&x.paths_b, path_bytes));
      x.paths_a = h->D.paths;
      x.c = c;
      h->paths_gen++;
    } catch (...) {
      x.c = c;  // so that detach_comm releases what was created
      x.paths_a = h->D.paths;
      detach_comm(h);
      throw;
    }
  });
}

int pmaf_winners_wait(pmaf_planner *h, const double **records, size_t *n_doubles) {
  return guarded([&] {
    REQUIRE(h, "pmaf_winners_wait: NULL handle");
    if (!h->x.c) fail(PMAF_ERR_STATE, "pmaf_winners_wait: no communicator attached (pmaf_attach_comm)");
    h->use_device();
    finish_exchanges(h);
    if (h->x.failed) fail(PMAF_ERR_DEVICE, "pmaf_winners_wait: the last winner exchange failed (no table)");
    if (records) *records = h->x.slot[h->x.cur].h_recv;
    if (n_doubles) *n_doubles = (size_t)h->D.P * winner_rec(h) * (size_t)h->x.c->world;
  });
}

void *pmaf_winners_device(pmaf_planner *h) { return h ? (void *)h->x.slot[h->x.cur].d_recv : nullptr; }

int pmaf_get_exchange_times_us(pmaf_planner *h, double *out, int32_t max_n, int32_t *n) {
  return guarded([&] {
    REQUIRE(h && n, "pmaf_get_exchange_times_us: NULL argument");
    std::vector<double> &v = h->x.ag_us;
    const size_t k = (out && max_n > 0) ? std::min(v.size(), (size_t)max_n) : 0;
    for (size_t i = 0; i < k; i++) out[i] = v[i];
    *n = (int32_t)k;
    v.clear();
  });
}

// ---- peer mailboxes (include/pmaf.h) ----
int pmaf_peer_export(pmaf_planner *h, int32_t world, void *handle_out) {
  return guarded([&] {
    REQUIRE(h && handle_out, "pmaf_peer_export: NULL argument");
    REQUIRE(world >= 1 && world <= PMAF_PEER_MAX_WORLD, "pmaf_peer_export: need 1 <= world <= 64");
    h->use_device();
    sync(h);
    peer_disconnect(h);
    pmaf_planner::Peer &pr = h->peer;
    const size_t bytes = sizeof(double) * peer_inbox_doubles(world, h->D.P);
    // fine-grained device memory: stores of other agents (peer GPUs over xGMI) become visible to this GPU's
    // system-scope loads without a kernel boundary; plain device memory as the fall-back
    hipError_t e = hipExtMallocWithFlags((void **)&pr.inbox, bytes, hipDeviceMallocFinegrained);
    pr.inbox_fine = e == hipSuccess;
    if (e != hipSuccess) { (void)hipGetLastError(); HIP_CHECK(hipMalloc((void **)&pr.inbox, bytes)); }
    {
      // sequence numbers start at -1 (no header yet)
      std::vector<double> init(peer_inbox_doubles(world, h->D.P), 0.0);
      for (size_t i = 8; i < init.size(); i += PMAF_PEER_SLOT) init[i] = -1.0;
      HIP_CHECK(hipMemcpy(pr.inbox, init.data(), bytes, hipMemcpyHostToDevice));
    }
    pr.world = world;
    PeerHandleBlob b{};
    b.magic = kPeerMagic; b.pid = (int64_t)getpid(); b.ptr = (uint64_t)(uintptr_t)pr.inbox;
    b.world = world; b.P = h->D.P; b.device = h->device;
    pci_id_of(h->device, b.pci);
    if (world > 1) {
      e = hipIpcGetMemHandle(&b.ipc, pr.inbox);
      if (e != hipSuccess && pr.inbox_fine) {   // this runtime does not export fine-grained memory: plain device memory
        (void)hipGetLastError();
        (void)hipFree(pr.inbox); pr.inbox = nullptr; pr.inbox_fine = false;
        HIP_CHECK(hipMalloc((void **)&pr.inbox, bytes));
        std::vector<double> init(peer_inbox_doubles(world, h->D.P), 0.0);
        for (size_t i = 8; i < init.size(); i += PMAF_PEER_SLOT) init[i] = -1.0;
        HIP_CHECK(hipMemcpy(pr.inbox, init.data(), bytes, hipMemcpyHostToDevice));
        b.ptr = (uint64_t)(uintptr_t)pr.inbox;
        e = hipIpcGetMemHandle(&b.ipc, pr.inbox);
      }
      if (e != hipSuccess) throw HipError{e, "hipIpcGetMemHandle (peer inbox)", __FILE__, __LINE__};
    }
    b.fine = pr.inbox_fine ? 1 : 0;   // (pmaf_peer_connect refuses cross-device peers of a plain-memory inbox)
    std::memcpy(handle_out, &b, sizeof(b));
  });
}

int pmaf_peer_connect(pmaf_planner *h, int32_t world, int32_t rank, const void *handles) {
  return guarded([&] {
    REQUIRE(h && handles, "pmaf_peer_connect: NULL argument");
    pmaf_planner::Peer &pr = h->peer;
    REQUIRE(pr.inbox && !pr.on, "pmaf_peer_connect: call pmaf_peer_export first (once per connection)");
    REQUIRE(world == pr.world && rank >= 0 && rank < world, "pmaf_peer_connect: world differs from pmaf_peer_export's, or bad rank");
    h->use_device();
    sync(h);
    const PeerHandleBlob *hb = static_cast<const PeerHandleBlob *>(handles);
    pr.mapped.assign(world, nullptr);
    pr.opened.assign(world, 0);
    for (int r = 0; r < world; r++) {
      const PeerHandleBlob &b = hb[r];
      REQUIRE(b.magic == kPeerMagic, "pmaf_peer_connect: not a handle of pmaf_peer_export");
      REQUIRE(b.world == world && b.P == h->D.P, "pmaf_peer_connect: every rank must export for the same world and hold the same number of populations");
      if (r != rank) {
        // a peer on ANOTHER GPU stores into / is stored into over xGMI while the kernels run: both inboxes must be
        // fine-grained memory (plain device memory does not make another agent's stores visible to a running kernel --
        // the in-kernel poll would time out every tick with no hint of the cause)
        int32_t mine[3];
        pci_id_of(h->device, mine);
        const bool same_gpu = mine[0] == b.pci[0] && mine[1] == b.pci[1] && mine[2] == b.pci[2] && mine[1] >= 0;
        if (!same_gpu && !(pr.inbox_fine && b.fine))
          fail(PMAF_ERR_DEVICE, "pmaf_peer_connect: a peer on another GPU needs fine-grained inboxes on both sides, and this "
                                "runtime could only export plain device memory (pmaf_peer_info); use the winner-record "
                                "exchange (pmaf_attach_comm) for the coupling instead");
      }
      if (r == rank) {
        REQUIRE(b.pid == (int64_t)getpid() && b.ptr == (uint64_t)(uintptr_t)pr.inbox, "pmaf_peer_connect: handles[rank] is not this handle's own export");
        pr.mapped[r] = pr.inbox;
      } else if (b.pid == (int64_t)getpid()) {
        // another handle of this process (several "ranks" in one process: tests, one host driving several GPUs)
        if (b.device != h->device) {
          hipError_t e = hipDeviceEnablePeerAccess(b.device, 0);
          if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) throw HipError{e, "hipDeviceEnablePeerAccess (peer inbox)", __FILE__, __LINE__};
          (void)hipGetLastError();
        }
        pr.mapped[r] = reinterpret_cast<double *>((uintptr_t)b.ptr);
      } else {
        void *p = nullptr;
        HIP_CHECK(hipIpcOpenMemHandle(&p, b.ipc, hipIpcMemLazyEnablePeerAccess));
        pr.mapped[r] = static_cast<double *>(p);
        pr.opened[r] = 1;
      }
    }
    pr.rank = rank;
    const int P = h->D.P;
    HIP_CHECK(hipMalloc((void **)&pr.d_view, sizeof(PeerView)));
    HIP_CHECK(hipMalloc((void **)&pr.d_couple, sizeof(int32_t) * 2 * P));
    HIP_CHECK(hipMalloc((void **)&pr.d_radius, sizeof(double) * P));
    pr.couple_h.assign(2 * (size_t)P, -1);
    pr.radius_h.assign(P, 0.0);
    HIP_CHECK(hipMemcpy(pr.d_couple, pr.couple_h.data(), sizeof(int32_t) * 2 * P, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pr.d_radius, pr.radius_h.data(), sizeof(double) * P, hipMemcpyHostToDevice));
    int khz = 0;
    HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device));
    if (khz <= 0) khz = 100000;
    pr.us_per_tick = 1e3 / (double)khz;
    double timeout_s = 2.0;
    { const char *to = getenv("PMAF_PEER_TIMEOUT_S"); if (to && atof(to) > 0.0) timeout_s = atof(to); }
    // the in-kernel wait for a peer's header must end before the host's wait for the tick does (PMAF_TICK_TIMEOUT_S):
    // otherwise a late peer is reported as a hung device and the tick is abandoned with its kernel still waiting
    if (timeout_s > 0.5 * h->tick_timeout_s) timeout_s = 0.5 * h->tick_timeout_s;
    PeerView v{};
    v.world = world; v.rank = rank; v.P = P;
    v.inbox = pr.inbox;
    for (int r = 0; r < world; r++) v.peer[r] = pr.mapped[r];
    v.couple = pr.d_couple; v.couple_radius = pr.d_radius;
    v.timeout_ticks = (unsigned long long)(timeout_s * 1e3 * (double)khz);
    HIP_CHECK(hipMemcpy(pr.d_view, &v, sizeof(v), hipMemcpyHostToDevice));
    pr.tick = 0;
    pr.on = true;
    h->live_resident.clear();
  });
}

int pmaf_peer_couple(pmaf_planner *h, int32_t pop, int32_t src_rank, int32_t src_pop, double radius, const double *init_pos) {
  return guarded([&] {
    REQUIRE(h, "pmaf_peer_couple: NULL handle");
    pmaf_planner::Peer &pr = h->peer;
    if (!pr.on) fail(PMAF_ERR_STATE, "pmaf_peer_couple: no peer mailboxes connected (pmaf_peer_connect)");
    REQUIRE(pop >= 0 && pop < h->D.P, "pmaf_peer_couple: bad population");
    h->use_device();
    sync(h);
    if (src_rank >= 0) {
      REQUIRE(src_rank < pr.world && src_pop >= 0 && src_pop < h->D.P, "pmaf_peer_couple: bad source rank / population");
      REQUIRE(!(src_rank == pr.rank && src_pop == pop), "pmaf_peer_couple: a population cannot be coupled to itself");
      check_range(&radius, 1, "pmaf_peer_couple: radius");
      if (init_pos) {
        if (pr.tick != 0) fail(PMAF_ERR_STATE, "pmaf_peer_couple: init_pos can only be given before the first pmaf_tick after pmaf_peer_connect");
        check_range(init_pos, 3, "pmaf_peer_couple: init_pos");
        // header "0" of the source population in this rank's own inbox (parity slot 0; its first real writer is the
        // source's tick 2, which needs this rank's tick 1 first)
        double slot[PMAF_PEER_SLOT] = {0};
        slot[4] = init_pos[0]; slot[5] = init_pos[1]; slot[6] = init_pos[2]; slot[8] = 0.0;
        slot[9] = slot[10] = -2.0;   // host-written header: the publisher's own coupling is not known here (k_manager's mutuality check skips it)
        HIP_CHECK(hipMemcpy(pr.inbox + (((size_t)0 * pr.world + src_rank) * h->D.P + src_pop) * PMAF_PEER_SLOT, slot,
                            sizeof(slot), hipMemcpyHostToDevice));
      }
    }
    pr.couple_h[2 * pop] = src_rank < 0 ? -1 : src_rank;
    pr.couple_h[2 * pop + 1] = src_rank < 0 ? -1 : src_pop;
    pr.radius_h[pop] = src_rank < 0 ? 0.0 : radius;
    HIP_CHECK(hipMemcpy(pr.d_couple, pr.couple_h.data(), sizeof(int32_t) * 2 * h->D.P, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pr.d_radius, pr.radius_h.data(), sizeof(double) * h->D.P, hipMemcpyHostToDevice));
  });
}

int pmaf_peer_disconnect(pmaf_planner *h) {
  return guarded([&] {
    REQUIRE(h, "pmaf_peer_disconnect: NULL handle");
    h->use_device();
    sync(h);
    peer_disconnect(h);
  });
}

int pmaf_peer_read(pmaf_planner *h, double *headers, double *seq) {
  return guarded([&] {
    REQUIRE(h, "pmaf_peer_read: NULL handle");
    pmaf_planner::Peer &pr = h->peer;
    if (!pr.on) fail(PMAF_ERR_STATE, "pmaf_peer_read: no peer mailboxes connected (pmaf_peer_connect)");
    h->use_device();
    const int P = h->D.P;
    std::vector<double> box(peer_inbox_doubles(pr.world, P));
    HIP_CHECK(hipMemcpy(box.data(), pr.inbox, sizeof(double) * box.size(), hipMemcpyDeviceToHost));
    for (int r = 0; r < pr.world; r++)
      for (int p = 0; p < P; p++) {
        const double *s0 = box.data() + (((size_t)0 * pr.world + r) * P + p) * PMAF_PEER_SLOT;
        const double *s1 = box.data() + (((size_t)1 * pr.world + r) * P + p) * PMAF_PEER_SLOT;
        const double *s = s1[8] > s0[8] ? s1 : s0;   // the newer of the two parity slots
        if (headers) std::memcpy(headers + ((size_t)r * P + p) * PMAF_WINNER_HDR, s, sizeof(double) * PMAF_WINNER_HDR);
        if (seq) seq[(size_t)r * P + p] = s[8];
      }
  });
}

int pmaf_get_peer_times_us(pmaf_planner *h, double *wait_us, double *publish_us, int32_t max_n, int32_t *n) {
  return guarded([&] {
    REQUIRE(h && n, "pmaf_get_peer_times_us: NULL argument");
    pmaf_planner::Peer &pr = h->peer;
    const size_t k = max_n > 0 ? std::min(pr.wait_us.size(), (size_t)max_n) : 0;
    for (size_t i = 0; i < k; i++) {
      if (wait_us) wait_us[i] = pr.wait_us[i];
      if (publish_us) publish_us[i] = pr.pub_us[i];
    }
    *n = (int32_t)k;
    pr.wait_us.clear();
    pr.pub_us.clear();
  });
}

int pmaf_peer_info(pmaf_planner *h, int32_t *fine_grained, int32_t *world) {
  return guarded([&] {
    REQUIRE(h, "pmaf_peer_info: NULL handle");
    if (!h->peer.inbox) fail(PMAF_ERR_STATE, "pmaf_peer_info: no inbox (pmaf_peer_export)");
    if (fine_grained) *fine_grained = h->peer.inbox_fine ? 1 : 0;
    if (world) *world = h->peer.world;
  });
}

}  // extern "C"
