// vgicp_multi.hip — the in-process multi-device context: ONE caller thread, 1-16 sub-contexts.
//
// The reference's caller is one process and one thread (src/main.cpp:68-70 runs Odometry::run on the main thread,
// src/ErrorStateKF.cpp:130 calls icp_->align, src/Odometry.cpp:79,86 the map update), so "ICP::align unchanged" and
// "partition the scan across 8 GPUs" (vgicp_create(const int* device_ids, int n_devices, ...), 8(e))
// only hold together if ONE handle drives every device.  A multi-device context is that handle:
//   * every device holds a replica of the voxel map: upsert / erase / insert / evict batches go to all replicas
//     (in parallel, one worker thread per extra device, each batch over the device's own PCIe link);
//   * vgicp_align shards the scan by contiguous point blocks ([r n / G, (r + 1) n / G), rank order = device order),
//     every device uploads its own shard and runs the SAME single persistent launch (the MULTI instantiation of
//     persistent_kernel): the rank rows cross xGMI through mailboxes that the kernels themselves write, the merge of
//     src/Registration.cpp:71-75 across devices — here the mailboxes are wired by plain pointers after
//     hipDeviceEnablePeerAccess (one address space: no IPC handles, no second process, no RCCL, no torch);
//   * device_ids may repeat a device ({0, 0, 0, 0}): the sub-contexts then split that device's compute units
//     (256 / multiplicity workgroups each) — the arrangement the 1-GPU test boxes can run;
//   * when an in-kernel wait gives up (or the caller asks for VGICP_FLAG_PROFILE / VGICP_FLAG_NO_PERSISTENT) the
//     align runs as one launch per round on every device with the rank rows added ON THE HOST in the mailbox
//     order — every sub-context's launch has ended when its thread returns, so the outcome is known to the one
//     process without any verdict protocol, the mailboxes are re-armed, and the single launch is tried again after
//     a few aligns.  No CPU arithmetic beyond that 28-value sum; no oracle; no fallback for a missing device.
// Which sub-context holds what of the resident scan is tracked here (a shard each after an upload; the whole
// prepared scan on device 0 after vgicp_scan_prepare, dealt out to the others by peer copies before the align).
#include <atomic>
#include <functional>

#include "vgicp_context.h"

namespace {

// One extra host thread per extra device.  A job is posted by the caller's thread and run with the worker's device
// current; the worker spins for a short while after a job (the next call of a frame follows within microseconds)
// and then sleeps on a condition variable.
struct Worker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::atomic<uint64_t> posted{0}, finished{0};
  std::function<int()> job;
  int result = VGICP_OK;
  bool quit = false;
  int device = 0;
  // what this thread's calls into the module have cost (vgicp_get_frame_stats): totals, published after every job
  std::atomic<uint64_t> launches{0}, copies{0}, syncs{0};

  void run() {
    (void)hipSetDevice(device);
    uint64_t seen = 0;
    for (;;) {
      bool have = false;
      for (int spins = 0; spins < 20000 && !have; ++spins) {
        have = posted.load(std::memory_order_acquire) != seen;
        if (!have) __builtin_ia32_pause();
      }
      if (!have) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return quit || posted.load(std::memory_order_acquire) != seen; });
        if (quit) return;
      }
      ++seen;
      result = job();
      launches.store(vgicp::g_kernel_launches, std::memory_order_relaxed);
      copies.store(g_copy_ops, std::memory_order_relaxed);
      syncs.store(g_sync_ops, std::memory_order_relaxed);
      finished.store(seen, std::memory_order_release);
    }
  }
  void post(std::function<int()> fn) {
    {
      std::lock_guard<std::mutex> lk(m);
      job = std::move(fn);
      posted.fetch_add(1, std::memory_order_release);
    }
    cv.notify_one();
  }
  int wait() {
    const uint64_t want = posted.load(std::memory_order_relaxed);
    for (uint32_t spins = 0; finished.load(std::memory_order_acquire) != want; ++spins) {
      if (spins < 200000) __builtin_ia32_pause();
      else std::this_thread::yield();
    }
    return result;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
    }
    cv.notify_one();
    if (th.joinable()) th.join();
  }
};

enum class Resident { None, Sharded, PreparedWhole, PreparedDealt };
constexpr int kGroupCooldownAligns = 8;

}  // namespace

struct vgicp_multi {
  int n = 0;
  std::vector<vgicp_ctx*> subs;
  std::vector<Worker*> workers;   // [r] for r >= 1; the caller's thread is rank 0's
  bool mailboxes = false;         // the device-initiated exchange is wired
  int cooldown = 0;               // aligns left on the host-summed loop after an in-kernel wait gave up
  uint64_t launches = 0, fallbacks = 0;
  bool verbose = false;           // VGICP_VERBOSE, read when the context is created
  mutable std::string status_text;   // vgicp_peer_status: composed when asked for
  std::string last_fallback;      // why the last align that left the mailboxes did
  // the resident scan
  Resident resident = Resident::None;
  size_t n_total = 0;
  std::vector<size_t> lo, hi;
  double prep_voxel = 0.0;
  bool prep_pending = false;      // vgicp_scan_prepare_async on device 0: size not read yet
  uint64_t scan_generation = 0;   // replacements of the resident scan as the CALLER sees it (dealing it out is not one)
  // whole-scan AoS copies for the map insertion on the devices that hold a shard only (points 3 cap, then covs 9 cap)
  std::vector<DeviceBuf<double>> d_full;
  std::vector<size_t> full_cap;
  std::vector<EventHandle> ev_gather;
  uint64_t stat_launches0 = 0, stat_copies0 = 0, stat_syncs0 = 0;   // caller's thread
  std::vector<uint64_t> w_launches0, w_copies0, w_syncs0;           // worker threads
};

namespace {

void shard_bounds(vgicp_multi* g, size_t n) {
  const size_t G = (size_t)g->n, base = n / G, extra = n % G;
  g->lo.assign(G, 0);
  g->hi.assign(G, 0);
  for (size_t r = 0; r < G; ++r) {
    g->lo[r] = r * base + std::min(r, extra);
    g->hi[r] = g->lo[r] + base + (r < extra ? 1 : 0);
  }
  g->n_total = n;
}

// fn(rank) on every sub-context at once: ranks >= 1 on their worker threads, rank 0 on the caller's.
// Returns the first status that is not OK (the parent context carries that sub-context's message).
int run_all(vgicp_ctx* parent, const std::function<int(int)>& fn, std::vector<int>* all = nullptr) {
  vgicp_multi* g = parent->multi;
  for (int r = 1; r < g->n; ++r) g->workers[(size_t)r]->post([&fn, r] { return fn(r); });
  std::vector<int> rc((size_t)g->n, VGICP_OK);
  rc[0] = fn(0);
  for (int r = 1; r < g->n; ++r) rc[(size_t)r] = g->workers[(size_t)r]->wait();
  if (all) *all = rc;
  for (int r = 0; r < g->n; ++r)
    if (rc[(size_t)r] != VGICP_OK) {
      parent->err = "device " + std::to_string(g->subs[(size_t)r]->device) + " (rank " + std::to_string(r) + "): " + g->subs[(size_t)r]->err;
      return rc[(size_t)r];
    }
  return VGICP_OK;
}

int sub_fail(vgicp_ctx* parent, vgicp_ctx* sub, int rc) {
  if (rc != VGICP_OK) parent->err = sub->err;
  return rc;
}

int ensure_full(vgicp_ctx* parent, int r, size_t n) {
  vgicp_multi* g = parent->multi;
  if (n <= g->full_cap[(size_t)r] && g->d_full[(size_t)r]) return VGICP_OK;
  VG_HIP(parent, hipSetDevice(g->subs[(size_t)r]->device));
  if (g->d_full[(size_t)r]) VG_HIP(parent, hipStreamSynchronize(g->subs[(size_t)r]->stream));
  g->full_cap[(size_t)r] = 0;
  const size_t cap = std::max<size_t>(n + n / 4, 1024);
  VG_HIP(parent, g->d_full[(size_t)r].alloc(cap * kScanPlanes * sizeof(double)));
  g->full_cap[(size_t)r] = cap;
  return VGICP_OK;
}

int copy_between(vgicp_ctx* parent, vgicp_ctx* dst_ctx, double* dst, const vgicp_ctx* src_ctx, const double* src, size_t bytes) {
  if (bytes == 0) return VGICP_OK;
  if (dst_ctx->device != src_ctx->device) {
    ++g_copy_ops;
    VG_HIP(parent, hipMemcpyPeerAsync(dst, dst_ctx->device, src, src_ctx->device, bytes, dst_ctx->stream));
  } else {
    VG_HIP(parent, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, dst_ctx->stream));
  }
  return VGICP_OK;
}

// The whole prepared scan sits on device 0: its size becomes known (one synchronisation if the preparation was only
// enqueued), every other device adopts its shard by a peer copy, device 0 keeps the first shard as a prefix.
int deal_prepared(vgicp_ctx* parent) {
  vgicp_multi* g = parent->multi;
  vgicp_ctx* lead = g->subs[0];
  int rc = vgicp_internal::settle_context(lead);
  if (rc != VGICP_OK) return sub_fail(parent, lead, rc);
  g->prep_pending = false;
  if (!lead->scan_ready) return fail(parent, VGICP_ERR_NOT_READY, "no scan resident");
  shard_bounds(g, lead->n);
  const double* whole_pts = lead->d_scan_aos;
  const double* whole_cov = lead->d_scan_aos + 3 * lead->scan_capacity;
  for (int r = 1; r < g->n; ++r) {
    const size_t lo = g->lo[(size_t)r], cnt = g->hi[(size_t)r] - lo;
    rc = vgicp_internal::adopt_device_scan(g->subs[(size_t)r], lead->device, whole_pts + 3 * lo, whole_cov + 9 * lo, cnt,
                                           g->prep_voxel, nullptr);
    if (rc != VGICP_OK) return sub_fail(parent, g->subs[(size_t)r], rc);
  }
  lead->n = (uint32_t)g->hi[0];   // the first shard is a prefix of the planes device 0 already holds
  g->resident = Resident::PreparedDealt;
  return VGICP_OK;
}

// The facts plan_align decides a GROUP's align by (vgicp_peer_status: with no flags, one round — the next plain align).
AlignFacts group_facts(const vgicp_multi* g, uint32_t flags, int max_iteration) {
  AlignFacts f = call_facts(AlignCall::Group, flags, max_iteration);
  f.mailboxes = g->mailboxes;
  // the single launch needs the persistent kernel on EVERY device (VGICP_PERSISTENT=0, or a workgroup that does not fit a
  // compute unit, leaves a sub-context on the launch-per-round loop)
  f.persistent_enabled = true;
  for (const vgicp_ctx* sub : g->subs) f.persistent_enabled = f.persistent_enabled && sub->persistent_enabled;
  f.cooldown = g->cooldown;
  return f;
}

// What a give-up costs the group (its sub-contexts neither cool down nor announce anything: align_persistent).
void note_fallback(vgicp_ctx* parent, const char* why) {
  vgicp_multi* g = parent->multi;
  ++g->fallbacks;
  g->cooldown = kGroupCooldownAligns;
  g->last_fallback = why;
  if (g->fallbacks == 1 || g->verbose)
    std::fprintf(stderr, "[vgicp] multi-device align: %s (fallback #%llu): this align and the next %d run one launch per round with "
                 "the devices' rows added on the host\n", why, (unsigned long long)g->fallbacks, kGroupCooldownAligns);
}

int upload_shards(vgicp_ctx* parent, const double* points, const double* covs) {
  vgicp_multi* g = parent->multi;
  return run_all(parent, [&](int r) {
    const size_t lo = g->lo[(size_t)r], cnt = g->hi[(size_t)r] - lo;
    vgicp_ctx* sub = g->subs[(size_t)r];
    sub->upload_whole_hint = g->hi[(size_t)g->n - 1] * kScanPlanes * sizeof(double);   // staged or direct: the caller's whole buffer decides
    const int rc_up = vgicp_scan_upload(sub, cnt, cnt ? points + 3 * lo : nullptr, cnt ? covs + 9 * lo : nullptr);
    sub->upload_whole_hint = 0;
    return rc_up;
  });
}

// The align itself.  points / covs == nullptr: every sub-context holds its shard already; otherwise the shards
// (bounds in g->lo / g->hi) go up first — on the single-launch path upload, packing and launch are ENQUEUED by each
// device's thread and synchronised once, as vgicp_align does on one device.
int align_shards(vgicp_ctx* parent, const double* points, const double* covs, const double guess[16], const vgicp_params* params,
                 double out_pose[16], vgicp_stats* stats) {
  vgicp_multi* g = parent->multi;
  const double t0 = now_seconds();
  if (!params) return fail(parent, VGICP_ERR_BAD_ARGUMENT, "params is NULL");
  // without the persistent kernel everywhere the host-summed loop is the path, not a fallback — nothing is counted,
  // announced or re-wired, and no device waits for a peer that will never publish
  const AlignPlan plan = plan_align(group_facts(g, params->flags, params->max_iteration));
  const bool single = plan.path == AlignPath::Persistent;
  g->cooldown -= plan.cooldown_drop;
  if (single) {
    // no allocation between the launches: a sub-context that has to grow its buffers (the scan's for a shard that comes
    // up with this call, the log) does so now, while nobody's persistent kernel is running (hipFree waits for the whole
    // device; on a shared device that would be a neighbour's launch, which in turn waits for this sub-context's)
    auto shard = [&](int r) { return points ? g->hi[(size_t)r] - g->lo[(size_t)r] : (size_t)g->subs[(size_t)r]->n; };
    bool grow = false;
    for (int r = 0; r < g->n; ++r) grow = grow || vgicp_internal::align_needs_allocation(g->subs[(size_t)r], shard(r), params->max_iteration);
    if (grow) {
      const int rc = run_all(parent, [&](int r) { return vgicp_internal::reserve_for_align(g->subs[(size_t)r], shard(r), params->max_iteration); });
      if (rc != VGICP_OK) return rc;
    }
  }
  if (single) {
    std::vector<double> pose((size_t)g->n * 16, 0.0);
    std::vector<vgicp_stats> st((size_t)g->n);
    for (auto& s : st) std::memset(&s, 0, sizeof s);
    if (stats) { st[0].corr_count = stats->corr_count; st[0].normal_eq = stats->normal_eq; st[0].kernel_ms = stats->kernel_ms; }
    std::vector<int> rcs;
    ++g->launches;
    (void)run_all(parent, [&](int r) {
      vgicp_ctx* sub = g->subs[(size_t)r];
      if (!points) return vgicp_align_resident(sub, guess, params, pose.data() + 16 * (size_t)r, &st[(size_t)r]);
      const size_t lo = g->lo[(size_t)r], cnt = g->hi[(size_t)r] - lo;
      sub->upload_whole_hint = g->hi[(size_t)g->n - 1] * kScanPlanes * sizeof(double);   // staged or direct: the caller's whole buffer decides
      const int rc_sub = vgicp_align(sub, cnt, cnt ? points + 3 * lo : nullptr, cnt ? covs + 9 * lo : nullptr, guess, params,
                                     pose.data() + 16 * (size_t)r, &st[(size_t)r]);
      sub->upload_whole_hint = 0;
      return rc_sub;
    }, &rcs);
    if (points) g->resident = Resident::Sharded;   // whatever the outcome below, the shards are up
    bool need_loop = false;
    for (int r = 0; r < g->n; ++r) need_loop = need_loop || rcs[(size_t)r] == vgicp_internal::kNeedGroupLoop;
    if (!need_loop) {
      int first_bad = VGICP_OK;
      for (int r = 0; r < g->n && first_bad == VGICP_OK; ++r)
        if (rcs[(size_t)r] != VGICP_OK) { first_bad = rcs[(size_t)r]; parent->err = g->subs[(size_t)r]->err; }
      // every device solved the same sums: anything but identical bits means the exchange is broken
      for (int r = 1; r < g->n && first_bad == VGICP_OK; ++r)
        if (std::memcmp(pose.data(), pose.data() + 16 * (size_t)r, 16 * sizeof(double)) != 0 || st[(size_t)r].iterations != st[0].iterations)
          return fail(parent, VGICP_ERR_HIP, "the devices of a multi-device align returned different poses (rank " + std::to_string(r) + ")");
      std::memcpy(out_pose, pose.data(), 16 * sizeof(double));
      if (stats) {
        stats->iterations = st[0].iterations;
        stats->converged = st[0].converged;
        stats->world_size = g->n;
        stats->launches = 1;
        stats->device_seconds = 0.0;
        for (int r = 0; r < g->n; ++r) stats->device_seconds = std::max(stats->device_seconds, st[(size_t)r].device_seconds);
        stats->seconds = now_seconds() - t0;
      }
      return first_bad;
    }
    // Some device's launch gave up.  Every launch has ended (each sub-context synchronised its stream before its
    // thread returned): re-arm all mailboxes from scratch and run this align with the rows added on the host.
    note_fallback(parent, "an in-kernel wait for another device (or for a workgroup) gave up");
    const int rc = vgicp_internal::wire_mailboxes(g->subs.data(), g->n);
    if (rc != VGICP_OK) {
      g->mailboxes = false;
      parent->peer_status = "mailboxes could not be re-armed after a launch gave up: " + g->subs[0]->err + " (the devices' rows are added on the host)";
    }
  } else if (points) {
    const int rc = upload_shards(parent, points, covs);
    if (rc != VGICP_OK) return rc;
    g->resident = Resident::Sharded;
  }
  const int rc = vgicp_internal::align_host_summed(g->subs.data(), g->n, guess, params, out_pose, stats);
  if (rc != VGICP_OK) {
    for (int r = 0; r < g->n; ++r)
      if (!g->subs[(size_t)r]->err.empty()) { parent->err = g->subs[(size_t)r]->err; break; }
  }
  if (stats) stats->seconds = now_seconds() - t0;
  return rc;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
extern "C" int vgicp_create_multi(const int* device_ids, int n_devices, vgicp_ctx** out) {
  if (!out) return fail(nullptr, VGICP_ERR_BAD_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (!device_ids || n_devices < 1 || n_devices > kMaxRanks)
    return fail(nullptr, VGICP_ERR_BAD_ARGUMENT, "device_ids must name 1 to 16 devices");
  if (n_devices == 1) return vgicp_create(device_ids[0], out);   // one device: the plain context IS the multi-device one
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0)
    return fail(nullptr, VGICP_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
  std::vector<int> multiplicity((size_t)count, 0);
  for (int r = 0; r < n_devices; ++r) {
    if (device_ids[r] < 0 || device_ids[r] >= count) return fail(nullptr, VGICP_ERR_BAD_ARGUMENT, "device_id out of range");
    ++multiplicity[(size_t)device_ids[r]];
  }
  vgicp_ctx* parent = new vgicp_ctx;
  parent->id = ++g_context_ids;   // never 0: vgicp_last_error tells this handle's text from a staging thread's by the id
  vgicp_multi* g = new vgicp_multi;
  parent->multi = g;
  g->n = n_devices;
  g->workers.assign((size_t)n_devices, nullptr);
  g->d_full.resize((size_t)n_devices);
  g->full_cap.assign((size_t)n_devices, 0);
  g->ev_gather.resize((size_t)n_devices);
  g->w_launches0.assign((size_t)n_devices, 0);
  g->w_copies0.assign((size_t)n_devices, 0);
  g->w_syncs0.assign((size_t)n_devices, 0);
  auto bail = [&](int rc, const std::string& text) {
    g_create_error = text;
    vgicp_multi_api::destroy(parent);
    return rc;
  };
  for (int r = 0; r < n_devices; ++r) {
    const int dev = device_ids[r], m = multiplicity[(size_t)dev];
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return bail(VGICP_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    // sub-contexts that share a device split its compute units: every workgroup of every one of them must be resident
    const uint32_t cap = m > 1 ? (uint32_t)std::max(1, std::min(prop.multiProcessorCount, kExchangeRows) / m) : 0u;
    vgicp_ctx* sub = nullptr;
    const int rc = vgicp_internal::create_context(dev, cap, &sub);
    if (rc != VGICP_OK) return bail(rc, g_create_error);
    sub->owner = g;
    // their uploads already run side by side (one thread per sub-context); a helper stream per sub-context on ONE
    // device would only make them share hardware queues with a neighbour's persistent launch
    if (m > 1) sub->upload_threads = 1;
    // ... and a workgroup of theirs plans with less than half a CU's LDS: launches of several queues that each need
    // WHOLE compute units were seen not to become resident side by side (4 and 8 queues, 150 KB per workgroup)
    if (m > 1) sub->persist_lds_budget = 64u * 1024u;
    g->subs.push_back(sub);
    if (hipSetDevice(dev) != hipSuccess || g->ev_gather[(size_t)r].create(false) != hipSuccess)
      return bail(VGICP_ERR_HIP, "hipEventCreate failed");
  }
  g->verbose = std::getenv("VGICP_VERBOSE") != nullptr;
  const char* how = std::getenv("VGICP_MULTI_EXCHANGE");   // "host": never use the mailboxes (developer / test aid)
  if (!(how && how[0] == 'h')) {
    const int rc = vgicp_internal::wire_mailboxes(g->subs.data(), n_devices);
    g->mailboxes = rc == VGICP_OK;
    if (!g->mailboxes && g->verbose)
      std::fprintf(stderr, "[vgicp] multi-device context: no device-initiated exchange (%s); the devices' rows are added on the host\n",
                   g->subs[0]->err.c_str());
    if (!g->mailboxes) {
      parent->peer_status = "mailboxes not wired: " + g->subs[0]->err + " (the devices' rows are added on the host)";
      for (vgicp_ctx* sub : g->subs) { sub->world_size = n_devices; sub->peer_world = n_devices; sub->peers_connected = false; }
    }
  } else {
    parent->peer_status = "mailboxes not wired: VGICP_MULTI_EXCHANGE=host";
  }
  for (int r = 0; r < n_devices; ++r) {   // ranks the sub-contexts report even without mailboxes
    g->subs[(size_t)r]->rank = r;
    g->subs[(size_t)r]->world_size = n_devices;
  }
  for (int r = 1; r < n_devices; ++r) {
    Worker* w = new Worker;
    w->device = device_ids[r];
    w->th = std::thread([w] { w->run(); });
    g->workers[(size_t)r] = w;
  }
  g->stat_launches0 = vgicp::g_kernel_launches;
  g->stat_copies0 = g_copy_ops;
  g->stat_syncs0 = g_sync_ops;
  (void)hipSetDevice(device_ids[0]);
  *out = parent;
  return VGICP_OK;
}

namespace vgicp_multi_api {

vgicp_ctx* first(const vgicp_ctx* ctx) { return ctx->multi->subs[0]; }

// What carries the per-round merge of the NEXT align, derived from the facts align_shards plans by (group_facts): "" only
// while the kernels' own mailboxes do.
const char* peer_status(const vgicp_ctx* ctx) {
  const vgicp_multi* g = ctx->multi;
  if (plan_align(group_facts(g, 0, 1)).path == AlignPath::Persistent) return "";
  if (!g->mailboxes) return ctx->peer_status.c_str();
  for (int r = 0; r < g->n; ++r)
    if (!g->subs[(size_t)r]->persistent_enabled) {
      g->status_text = "mailboxes wired, but device rank " + std::to_string(r) + " cannot run the single persistent launch "
                       "(VGICP_PERSISTENT=0 or its workgroup does not fit a compute unit): one launch per round, the devices' rows added on the host";
      return g->status_text.c_str();
    }
  g->status_text = "mailboxes wired, but " + g->last_fallback + " (fallback #" + std::to_string(g->fallbacks) + "): the next " +
                   std::to_string(g->cooldown) + " aligns run one launch per round with the devices' rows added on the host";
  return g->status_text.c_str();
}

void scan_replaced(vgicp_ctx* ctx) {   // a hook put its own scan on device 0: nothing is resident as far as the caller goes
  ++ctx->multi->scan_generation;
  ctx->multi->resident = Resident::None;
}

int destroy(vgicp_ctx* ctx) {
  vgicp_multi* g = ctx->multi;
  for (Worker* w : g->workers)
    if (w) { w->stop(); delete w; }
  for (size_t r = 0; r < g->subs.size(); ++r) {
    vgicp_ctx* sub = g->subs[r];
    (void)hipSetDevice(sub->device);
    if (sub->stream) (void)(hipStreamSynchronize)(sub->stream);
  }
  for (vgicp_ctx* sub : g->subs) {
    sub->owner = nullptr;
    vgicp_destroy(sub);
  }
  delete g;   // the group's own copies and events: every stream that used them was waited for above
  ctx->multi = nullptr;
  delete ctx;
  return VGICP_OK;
}

int device_info(const vgicp_ctx* ctx, char* name, size_t name_len, int32_t* cu_count, uint64_t* hbm_bytes) {
  const vgicp_multi* g = ctx->multi;
  if (name && name_len) {
    std::strncpy(name, g->subs[0]->arch.c_str(), name_len - 1);
    name[name_len - 1] = '\0';
  }
  // compute units and memory over the DISTINCT devices
  int32_t cus = 0;
  uint64_t hbm = 0;
  for (size_t r = 0; r < g->subs.size(); ++r) {
    bool seen = false;
    for (size_t q = 0; q < r; ++q) seen = seen || g->subs[q]->device == g->subs[r]->device;
    if (!seen) { cus += g->subs[r]->cu_count; hbm += g->subs[r]->hbm_bytes; }
  }
  if (cu_count) *cu_count = cus;
  if (hbm_bytes) *hbm_bytes = hbm;
  return VGICP_OK;
}

int get_counter(const vgicp_ctx* ctx, int which, uint64_t* value) {
  const vgicp_multi* g = ctx->multi;
  uint64_t v = 0;
  switch (which) {
    case VGICP_COUNTER_PERSISTENT_LAUNCHES: v = g->launches; break;
    case VGICP_COUNTER_PERSISTENT_FALLBACKS: v = g->fallbacks; break;
    case VGICP_COUNTER_UPLOAD_BYTES: for (const vgicp_ctx* s : g->subs) v += s->upload_bytes; break;
    case VGICP_COUNTER_UPLOAD_NANOSECONDS: for (const vgicp_ctx* s : g->subs) v = std::max<uint64_t>(v, (uint64_t)(s->upload_seconds * 1e9)); break;
    case VGICP_COUNTER_SCAN_GENERATION: v = g->scan_generation; break;
    case VGICP_COUNTER_UPLOAD_SLOW: for (const vgicp_ctx* s : g->subs) v += s->upload_slow; break;
    case VGICP_COUNTER_PREP_INDEFINITE: return sub_fail(const_cast<vgicp_ctx*>(ctx), g->subs[0], vgicp_get_counter(g->subs[0], which, value));
    default: return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "unknown counter");
  }
  *value = v;
  return VGICP_OK;
}

// ---- the replicated map: every batch goes to every replica ----
int map_reset(vgicp_ctx* ctx, double voxel_size, size_t capacity_hint) {
  vgicp_multi* g = ctx->multi;
  return run_all(ctx, [&](int r) { return vgicp_map_reset(g->subs[(size_t)r], voxel_size, capacity_hint); });
}
int map_upsert(vgicp_ctx* ctx, size_t n, const int32_t* keys, const double* means, const double* covs) {
  vgicp_multi* g = ctx->multi;
  // refused before any replica takes the batch (only the first keeps raw points: the others would accept it)
  if (g->subs[0]->raw_on) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the map keeps raw points (VGICP_OPTION_MAP_RAW_POINTS): a mirror batch carries none");
  return run_all(ctx, [&](int r) { return vgicp_map_upsert(g->subs[(size_t)r], n, keys, means, covs); });
}
int map_erase(vgicp_ctx* ctx, size_t n, const int32_t* keys) {
  vgicp_multi* g = ctx->multi;
  return run_all(ctx, [&](int r) { return vgicp_map_erase(g->subs[(size_t)r], n, keys); });
}
int map_size(const vgicp_ctx* ctx, size_t* voxels, size_t* table_slots) {
  vgicp_multi* g = ctx->multi;
  vgicp_ctx* parent = const_cast<vgicp_ctx*>(ctx);
  std::vector<size_t> v((size_t)g->n, 0), s((size_t)g->n, 0);
  const int rc = run_all(parent, [&](int r) { return vgicp_map_size(g->subs[(size_t)r], &v[(size_t)r], &s[(size_t)r]); });
  if (rc != VGICP_OK) return rc;
  for (int r = 1; r < g->n; ++r)
    if (v[(size_t)r] != v[0]) return fail(ctx, VGICP_ERR_HIP, "the map replicas of a multi-device context have diverged");
  if (voxels) *voxels = v[0];
  if (table_slots) *table_slots = s[0];
  return VGICP_OK;
}
int map_insert_scan(vgicp_ctx* ctx, size_t n, const double* points, const double* covs, const double transform[16],
                    size_t max_points_per_voxel, size_t* new_voxels) {
  vgicp_multi* g = ctx->multi;
  std::vector<size_t> fresh((size_t)g->n, 0);
  const int rc = run_all(ctx, [&](int r) {
    return vgicp_map_insert_scan(g->subs[(size_t)r], n, points, covs, transform, max_points_per_voxel, &fresh[(size_t)r]);
  });
  if (new_voxels) *new_voxels = fresh[0];
  return rc;
}
int map_evict(vgicp_ctx* ctx, const double position[3], double distance_threshold, size_t* removed) {
  vgicp_multi* g = ctx->multi;
  std::vector<size_t> gone((size_t)g->n, 0);
  const int rc = run_all(ctx, [&](int r) { return vgicp_map_evict(g->subs[(size_t)r], position, distance_threshold, &gone[(size_t)r]); });
  if (removed) *removed = gone[0];
  return rc;
}
int map_export(vgicp_ctx* ctx, size_t capacity, int32_t* keys, double* means, double* covs, uint64_t* counts, size_t* written) {
  return sub_fail(ctx, ctx->multi->subs[0], vgicp_map_export(ctx->multi->subs[0], capacity, keys, means, covs, counts, written));
}

// LocalMap::updateLocalMap for the scan that is resident: every replica needs the WHOLE scan in scan order (the
// insertion rule is order-dependent inside a voxel, include/ESKF_LIO/LocalMap.hpp:79-87), so a device that holds a
// shard only first gathers the others' shards (peer copies on its own stream).
int map_insert_resident(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, size_t* new_voxels, bool deferred) {
  vgicp_multi* g = ctx->multi;
  if (new_voxels) *new_voxels = 0;
  if (!transform) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  if (g->resident == Resident::None) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  vgicp_ctx* lead = g->subs[0];
  int rc = VGICP_OK;
  if (g->resident == Resident::PreparedWhole) {   // never dealt out (e.g. the first frame: no align): the size is on device 0
    rc = vgicp_internal::settle_context(lead);
    if (rc != VGICP_OK) return sub_fail(ctx, lead, rc);
    g->prep_pending = false;
    g->n_total = lead->n;
  }
  const size_t n = g->n_total;
  if (n == 0) return VGICP_OK;
  const bool prepared = g->resident != Resident::Sharded;
  const bool short_lists = prepared && insertion_lists_stay_short(lead->voxel_size, g->prep_voxel, lead->dev.insert_sort);
  std::vector<const double*> pts((size_t)g->n, nullptr), cov((size_t)g->n, nullptr);
  for (int r = 0; r < g->n; ++r) {
    vgicp_ctx* sub = g->subs[(size_t)r];
    if (prepared && r == 0) {   // device 0 holds the whole prepared scan already
      pts[0] = lead->d_scan_aos;
      cov[0] = lead->d_scan_aos + 3 * lead->scan_capacity;
      continue;
    }
    rc = ensure_full(ctx, r, n);
    if (rc != VGICP_OK) return rc;
    double* full = g->d_full[(size_t)r];
    const size_t cap = g->full_cap[(size_t)r];
    VG_HIP(ctx, hipSetDevice(sub->device));
    if (prepared) {
      rc = copy_between(ctx, sub, full, lead, lead->d_scan_aos, n * 3 * sizeof(double));
      if (rc == VGICP_OK) rc = copy_between(ctx, sub, full + 3 * cap, lead, lead->d_scan_aos + 3 * lead->scan_capacity, n * 9 * sizeof(double));
    } else {
      for (int q = 0; q < g->n && rc == VGICP_OK; ++q) {
        const vgicp_ctx* src = g->subs[(size_t)q];
        const size_t lo = g->lo[(size_t)q], cnt = g->hi[(size_t)q] - lo;
        rc = copy_between(ctx, sub, full + 3 * lo, src, src->d_scan_aos, cnt * 3 * sizeof(double));
        if (rc == VGICP_OK) rc = copy_between(ctx, sub, full + 3 * cap + 9 * lo, src, src->d_scan_aos + 3 * src->scan_capacity, cnt * 9 * sizeof(double));
      }
    }
    if (rc != VGICP_OK) return rc;
    VG_HIP(ctx, hipEventRecord(g->ev_gather[(size_t)r], sub->stream));
    pts[(size_t)r] = full;
    cov[(size_t)r] = full + 3 * cap;
  }
  // whatever a device enqueues next (the next frame's upload or preparation overwrites its scan) waits until every
  // other device has read what it needed
  for (int r = 0; r < g->n; ++r) {
    VG_HIP(ctx, hipSetDevice(g->subs[(size_t)r]->device));
    for (int q = 0; q < g->n; ++q)
      if (q != r && !(prepared && q == 0)) VG_HIP(ctx, hipStreamWaitEvent(g->subs[(size_t)r]->stream, g->ev_gather[(size_t)q], 0));
  }
  std::vector<size_t> fresh((size_t)g->n, 0);
  rc = run_all(ctx, [&](int r) {
    return vgicp_internal::map_insert_device(g->subs[(size_t)r], pts[(size_t)r], cov[(size_t)r], n, transform, max_points_per_voxel,
                                             short_lists, deferred, &fresh[(size_t)r]);
  });
  if (new_voxels) *new_voxels = fresh[0];
  return rc;
}

// ---- the scan ----
int scan_upload(vgicp_ctx* ctx, size_t n, const double* points, const double* covs) {
  vgicp_multi* g = ctx->multi;
  if (n > 0 && (!points || !covs)) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL scan pointer");
  shard_bounds(g, n);
  ++g->scan_generation;
  g->resident = Resident::None;
  g->prep_voxel = 0.0;
  g->prep_pending = false;
  const int rc = upload_shards(ctx, points, covs);
  if (rc == VGICP_OK) g->resident = Resident::Sharded;
  return rc;
}

int align(vgicp_ctx* ctx, size_t n, const double* points, const double* covs, const double guess[16],
          const vgicp_params* params, double out_pose[16], vgicp_stats* stats) {
  vgicp_multi* g = ctx->multi;
  if (n > 0 && (!points || !covs)) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL scan pointer");
  shard_bounds(g, n);   // every device its own shard, side by side, over its own link
  ++g->scan_generation;
  g->resident = Resident::None;
  g->prep_voxel = 0.0;
  g->prep_pending = false;
  static const double nothing[9] = {0.0};   // an empty scan still takes the upload path
  return align_shards(ctx, points ? points : nothing, covs ? covs : nothing, guess, params, out_pose, stats);
}

int align_resident(vgicp_ctx* ctx, const double guess[16], const vgicp_params* params, double out_pose[16], vgicp_stats* stats) {
  vgicp_multi* g = ctx->multi;
  if (g->resident == Resident::None) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  if (g->resident == Resident::PreparedWhole) {
    const int rc = deal_prepared(ctx);
    if (rc != VGICP_OK) return rc;
  }
  return align_shards(ctx, nullptr, nullptr, guess, params, out_pose, stats);
}

// vgicp_hip_batch.h on a multi-device context: every hypothesis is one point-sharded align over all devices, one after
// another (teams of one device's launch would have to share the mailboxes; not built)
int align_resident_batch(vgicp_ctx* ctx, size_t k, const double* guesses, const vgicp_params* params, double* out_poses,
                         vgicp_batch_stats* stats, int* first_bad) {
  return vgicp_internal::align_batch_sequential(ctx, k, guesses, params, out_poses, stats, /*loop_only=*/false, first_bad);
}
int align_batch_width(vgicp_ctx* ctx, size_t* hypotheses_per_launch) {
  if (ctx->multi->resident == Resident::None) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  *hypotheses_per_launch = 1;
  return VGICP_OK;
}

// CloudPreprocessor::process on device 0 (one sweep is one device's work: sort, octree, 30-NN), the result dealt out
// to the other devices right before the align.
int scan_prepare(vgicp_ctx* ctx, size_t n, const double* points, const double* point_time, size_t num_states,
                 const double* states, const double extrinsic[16], double voxel_size, int knn, size_t* kept,
                 int64_t* deskewed, bool deferred, uint64_t ticket) {
  vgicp_multi* g = ctx->multi;
  vgicp_ctx* lead = g->subs[0];
  ++g->scan_generation;
  g->resident = Resident::None;
  int rc;
  if (ticket) rc = vgicp_scan_prepare_staged_async(lead, ticket, num_states, states, extrinsic, voxel_size, knn);
  else if (deferred) rc = vgicp_scan_prepare_async(lead, n, points, point_time, num_states, states, extrinsic, voxel_size, knn);
  else rc = vgicp_scan_prepare(lead, n, points, point_time, num_states, states, extrinsic, voxel_size, knn, kept, deskewed);
  if (rc != VGICP_OK) return sub_fail(ctx, lead, rc);
  g->resident = Resident::PreparedWhole;
  g->prep_voxel = voxel_size;
  g->prep_pending = deferred;
  g->n_total = deferred ? 0 : lead->n;
  return VGICP_OK;
}

int scan_info(vgicp_ctx* ctx, size_t* kept, int64_t* deskewed, uint64_t* indefinite) {
  vgicp_multi* g = ctx->multi;
  if (kept) *kept = 0;
  if (deskewed) *deskewed = 0;
  if (indefinite) *indefinite = 0;
  if (g->resident == Resident::None) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident");
  if (g->resident == Resident::PreparedWhole) {
    const int rc = vgicp_scan_info(g->subs[0], kept, deskewed, indefinite);
    if (rc == VGICP_OK) { g->prep_pending = false; g->n_total = g->subs[0]->n; }
    return sub_fail(ctx, g->subs[0], rc);
  }
  if (g->resident == Resident::PreparedDealt) {   // device 0 still knows what its preparation found; its n is a shard now
    const int rc = vgicp_scan_info(g->subs[0], nullptr, deskewed, indefinite);
    if (kept) *kept = g->n_total;
    return sub_fail(ctx, g->subs[0], rc);
  }
  if (kept) *kept = g->n_total;
  return VGICP_OK;
}

int scan_download(vgicp_ctx* ctx, size_t capacity, double* points, double* covs, size_t* n) {
  vgicp_multi* g = ctx->multi;
  if (!n) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "n is NULL");
  *n = 0;
  if (g->resident == Resident::None) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload or vgicp_scan_prepare first");
  vgicp_ctx* lead = g->subs[0];
  if (g->resident == Resident::PreparedWhole) return sub_fail(ctx, lead, vgicp_scan_download(lead, capacity, points, covs, n));
  *n = g->n_total;
  if (g->n_total == 0 || (!points && !covs)) return VGICP_OK;
  if (capacity < g->n_total) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "capacity smaller than the resident scan");
  if (!points || !covs) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL output pointer");
  if (g->resident == Resident::PreparedDealt) {   // device 0 still holds all of it (its own shard is a prefix of the planes)
    int rc = vgicp_internal::settle_context(lead);
    if (rc != VGICP_OK) return sub_fail(ctx, lead, rc);
    // through the single-device entry point with the full count: its copies go through the context's page-locked arena
    // (a copy straight into the caller's pageable memory would let the runtime register those pages: the ~20 ms stall
    // when the caller frees them)
    const uint32_t shard = lead->n;
    lead->n = (uint32_t)g->n_total;
    size_t got = 0;
    rc = vgicp_scan_download(lead, capacity, points, covs, &got);
    lead->n = shard;
    return sub_fail(ctx, lead, rc);
  }
  return run_all(ctx, [&](int r) {
    const size_t lo = g->lo[(size_t)r], cnt = g->hi[(size_t)r] - lo;
    size_t got = 0;
    if (cnt == 0) return (int)VGICP_OK;
    return vgicp_scan_download(g->subs[(size_t)r], cnt, points + 3 * lo, covs + 9 * lo, &got);
  });
}

int get_frame_stats(vgicp_ctx* ctx, vgicp_frame_stats* out, int reset) {
  vgicp_multi* g = ctx->multi;
  // stage spans: device 0's (the preparation runs there; align and insertion run on every device side by side)
  const int rc = vgicp_get_frame_stats(g->subs[0], out, 0);
  if (rc != VGICP_OK) return sub_fail(ctx, g->subs[0], rc);
  uint64_t launches = vgicp::g_kernel_launches - g->stat_launches0, copies = g_copy_ops - g->stat_copies0, syncs = g_sync_ops - g->stat_syncs0;
  for (int r = 1; r < g->n; ++r) {
    const Worker* w = g->workers[(size_t)r];
    launches += w->launches.load() - g->w_launches0[(size_t)r];
    copies += w->copies.load() - g->w_copies0[(size_t)r];
    syncs += w->syncs.load() - g->w_syncs0[(size_t)r];
  }
  out->kernel_launches = launches;
  out->copies = copies;
  out->host_syncs = syncs;
  if (reset) {
    g->stat_launches0 = vgicp::g_kernel_launches;
    g->stat_copies0 = g_copy_ops;
    g->stat_syncs0 = g_sync_ops;
    for (int r = 1; r < g->n; ++r) {
      const Worker* w = g->workers[(size_t)r];
      g->w_launches0[(size_t)r] = w->launches.load();
      g->w_copies0[(size_t)r] = w->copies.load();
      g->w_syncs0[(size_t)r] = w->syncs.load();
    }
  }
  return VGICP_OK;
}

int set_option(vgicp_ctx* ctx, int option, int value) {
  vgicp_multi* g = ctx->multi;
  // the raw points are read from the first device only (vgicp_map_points_export, like vgicp_map_export): only it keeps them
  if (option == VGICP_OPTION_ROBUST_KERNEL || option == VGICP_OPTION_ROBUST_SCALE_MICRO || option == VGICP_OPTION_GATE_MICRO)
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the robust round (vgicp_hip_robust.h) runs on a single-device context only");
  if (option == VGICP_OPTION_MAP_RAW_POINTS) return sub_fail(ctx, g->subs[0], vgicp_set_option(g->subs[0], option, value));
  return run_all(ctx, [&](int r) { return vgicp_set_option(g->subs[(size_t)r], option, value); });
}

}  // namespace vgicp_multi_api
