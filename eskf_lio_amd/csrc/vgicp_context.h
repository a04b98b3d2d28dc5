// vgicp_context.h — the host-side context behind the C ABI (include/vgicp_hip.h), shared by vgicp_capi.hip (one
// device) and vgicp_multi.hip (one caller thread driving several devices).  Not part of the ABI: callers only ever
// see the opaque vgicp_ctx*.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <limits>
#include <memory>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vgicp_hip.h"
#include "../../include/vgicp_hip_map_points.h"
#include "../../include/vgicp_hip_batch.h"
#include "../../include/vgicp_hip_evaluate.h"
#include "../../include/vgicp_hip_robust.h"
#include "../../include/vgicp_hip_prior.h"
#include "../../include/vgicp_hip_points.h"
#include "../../include/vgicp_hip_map_gated.h"
#include "../../include/vgicp_hip_map_carve.h"
#include "../../include/vgicp_hip_map_rays.h"
#include "../../include/vgicp_hip_search_report.h"
#include "../../include/vgicp_hip_map_levels.h"
#include "../../include/vgicp_hip_map_locate.h"
#include "../../include/vgicp_hip_map_submap.h"
#include "../../include/vgicp_hip_map_checkpoint.h"
#include "../../include/vgicp_hip_map_merge.h"
#include "vgicp_device.h"
#include "vgicp_owned.h"
#include "vgicp_align_plan.h"
#include "vgicp_prepare_plan.h"
#include "vgicp_resident_plan.h"
#include "vgicp_map_plan.h"
#include "vgicp_points_plan.h"
#include "vgicp_levels_plan.h"
#include "vgicp_locate_plan.h"
#include "vgicp_submap_plan.h"
#include "vgicp_checkpoint_plan.h"
#include "vgicp_merge_plan.h"

using namespace vgicp;

// what a frame costs the host besides kernels: copies / memsets enqueued and synchronisations (vgicp_get_frame_stats)
namespace vgicp { extern thread_local uint64_t g_copy_ops, g_sync_ops; }
using vgicp::g_copy_ops;
using vgicp::g_sync_ops;
#define hipMemcpyAsync(...) (++g_copy_ops, hipMemcpyAsync(__VA_ARGS__))
#define hipMemsetAsync(...) (++g_copy_ops, hipMemsetAsync(__VA_ARGS__))
#define hipStreamSynchronize(...) (++g_sync_ops, hipStreamSynchronize(__VA_ARGS__))
#define hipEventSynchronize(...) (++g_sync_ops, hipEventSynchronize(__VA_ARGS__))

namespace vgicp {

// ---- the few RCCL entry points used, bound at run time so the library loads without RCCL ----
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[VGICP_UNIQUE_ID_BYTES]; } ncclUniqueId;
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(ncclUniqueId*) = nullptr;
  int (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  int (*CommDestroy)(ncclComm_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
constexpr int kNcclDouble = 8;  // ncclFloat64, rccl.h
constexpr int kNcclSum = 0;
constexpr int kNcclChar = 0;   // ncclInt8

extern thread_local std::string g_create_error;
// what vgicp_sweep_stage* report: those may run on another thread than the context's owner (who writes ctx->err), so
// their text lives with the calling thread; vgicp_last_error(ctx) returns it to that thread until it fails elsewhere
extern thread_local std::string g_stage_error;
// ... identified by the context's creation number, not by its address: a context destroyed on one thread and another
// allocated at the same address must not inherit a stale text that a third thread still keeps
extern thread_local uint64_t g_stage_error_ctx;
extern std::atomic<uint64_t> g_context_ids;

inline double now_seconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
// sequence numbers (scan_seq, prep_epoch, fetch_seq): 0 means "none yet" in every flag and header word, so it is skipped
inline uint32_t next_nonzero(uint32_t& seq) {
  if (++seq == 0) ++seq;
  return seq;
}

// words behind the counter block (d_ins_counters): [0] [1] the deferred insertion's running totals, [2] [3] the
// resident scan's symmetry verdicts, [4] [5] [6] the raw-point log (RawLog::ctr), [7] a deferred carve's rays, [8] [9] [10] a
// gated insertion's running totals (kGateCounters: matched, refused, not finite), [11] a deferred carve's removed voxels
// (include/vgicp_hip_map_carve.h).  The copies that bring the block to the host carry the first 2 / 4 / 6 / 8 words as
// before; all of them only while a gated insertion or a carve is pending
constexpr int kInsertWords = 12;
constexpr int kInsertWordsRaw = 8;    // up to the raw-point log's words
constexpr int kGateWord = 8;
constexpr int kCarveRaysWord = 7;
constexpr int kCarveRemovedWord = 11;
constexpr int kDefaultChunk = 4;
constexpr int kMaxChunksInFlight = 2;
static_assert(kPlanTeamsMax == (uint32_t)kTeamsMax, "vgicp_align_plan.h plans with the team kernel's width");
static_assert(kPlanDeskewMaxStates == kDeskewMaxStates, "vgicp_prepare_plan.h plans with the parallel deskew bounds' limit");
constexpr int kPersistentCooldownAligns = 8;  // aligns on the per-launch loop after the single launch gave up

// ---- ownership (vgicp_owned.h): the HIP calls behind the owners.  The ONLY place of the host code that allocates or
// frees device memory, page-locked memory, events and the stream ----
struct HipBackend {
  using error = hipError_t;
  static constexpr error ok = hipSuccess;
  using event = hipEvent_t;
  using stream = hipStream_t;
  // fine_grained: stores of another GPU's kernel become visible to this GPU's running kernel (the mailbox)
  static error device_alloc(void** p, size_t bytes, bool fine_grained) {
    return fine_grained ? hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained) : hipMalloc(p, bytes);
  }
  static void device_free(void* p) { (void)hipFree(p); }
  static error pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, 0); }
  static void pinned_free(void* p) { (void)hipHostFree(p); }
  static error pinned_alias(void** dev, void* host) { return hipHostGetDevicePointer(dev, host, 0); }
  static error event_create(event* e, bool timing) {
    return timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming);
  }
  static void event_destroy(event e) { (void)hipEventDestroy(e); }
  static error stream_create(stream* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
  static void stream_destroy(stream s) { (void)hipStreamDestroy(s); }
};
template <class T> using DeviceBuf = owned::DeviceBuf<T, HipBackend>;
template <class T> using PinnedBuf = owned::PinnedBuf<T, HipBackend>;
using EventHandle = owned::EventHandle<HipBackend>;
using StreamHandle = owned::StreamHandle<HipBackend>;

}  // namespace vgicp
using namespace vgicp;

// The host side of the scan upload (vgicp_align, vgicp_scan_upload): a crew of plain-memcpy threads.
// The caller's scan lives in pageable memory that the caller frees right after the call (the reference deep-copies a
// fresh cloud per frame, src/Registration.cpp:11).  Handing such a buffer to the runtime registers its pages with the
// driver, and the free() then takes every queue of the process off the device for ~20 ms (profiles/r10_sync_stall.txt);
// staging it through page-locked memory with copy COMMANDS cost 0.45 - 0.68 ms for 9.6 MB (25 commands of ~19 us).
// So: the crew — the caller's own thread plus `helpers` threads that make no HIP call — copies the scan into page-locked
// staging memory in units of pack_arena_unit() points and publishes every unit with a flag, and ONE kernel launch
// (pack_arena_kernel) reads the staging memory over PCIe behind them.  Measured (tools/micro/stage_crew_probe.hip,
// 2 x EPYC 9575F): one thread copies 9.6 MB from never-seen pages in 0.22 ms (43 GB/s), two in 0.13 - 0.15 ms; the kernel
// gets 54 GB/s out of the link; copy + transfer + packing overlapped: 0.19 - 0.20 ms with ONE helper, the link's rate.
// A helper spins for a short while after a job (the next frame's upload follows soon in a loop) and then sleeps.
struct CopyCrew {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv;
  std::atomic<uint32_t> gen{0};        // the job the helpers were last woken for
  // job number << 32 | next unit to take.  A job is OPEN from post() to finish(): finish() closes it (unit word ~0)
  // BEFORE the caller may write a field of the next job, so a thread that comes late to a job that is over can never
  // take a unit with the next job's fields half written (round 5's advisor reproduced exactly that with a unit count
  // that varies from job to job: its bounds check read the NEXT job's larger count, its compare-and-swap on the OLD
  // job's exhausted ticket succeeded).  A unit is taken by compare-and-swap, so a closed ticket is left alone.
  std::atomic<uint64_t> next{0};
  // job number << 32 | units of that job completed: a completion that lands after its job was given up (deadline) finds
  // another job's number here and is dropped instead of being counted for the job that follows
  std::atomic<uint64_t> finished{0};
  std::atomic<uint32_t> taken{0};      // units whose job fields a thread has read so far (see work())
  uint32_t job = 0;                    // jobs posted so far (the caller's thread only)
  bool quit = false;
  bool broken = false;                 // a helper missed finish()'s deadline: no helper is woken again (caller's thread only)
  // the job (written while no job is open, read only after a unit of THIS job was taken)
  const char* pts = nullptr;
  const char* cov = nullptr;
  char* apts = nullptr;
  char* acov = nullptr;
  uint32_t* flags = nullptr;
  uint32_t n = 0, unit = 0, seq = 0;
  std::atomic<uint32_t> units{0};      // read BEFORE a unit is taken (by a thread that may have come late to an older job): atomic
  uint32_t size_a = 24, size_b = 72;   // bytes per point of the two arrays (size_b = 0: one array only)
  void (*copy)(void*, const void*, size_t) = nullptr;
  // optional: the second array's units are written by this instead (dst = the unit's place, cnt points of size_b bytes
  // in src); what it returns is stored into the unit's flag line (word 1) before the flag: the form the unit was
  // staged in (the covariances of a scan upload: compact when all of a unit's are bitwise symmetric)
  uint32_t (*copy_b_form)(void*, const void*, size_t) = nullptr;
  static constexpr uint32_t kClosed = 0xFFFFFFFFu;

  void work(uint32_t my_job) {
    for (;;) {
      uint64_t v = next.load(std::memory_order_acquire);
      for (;;) {
        // closed (~0) or exhausted or another job's ticket: nothing to take.  The count may belong to a LATER job only
        // when this ticket is closed already, and then the compare-and-swap below cannot succeed.
        if ((uint32_t)(v >> 32) != my_job || (uint32_t)v >= units.load(std::memory_order_relaxed)) return;
        if (next.compare_exchange_weak(v, v + 1, std::memory_order_acq_rel, std::memory_order_acquire)) break;
      }
      const uint32_t u = (uint32_t)v;
      // the job was open when the unit was taken and stays open until the unit is delivered — unless finish() gives
      // up on this thread: everything it touches from here on is what the job was THEN, never a later job's fields
      const char *j_pts = pts, *j_cov = cov;
      char *j_apts = apts, *j_acov = acov;
      uint32_t* j_flags = flags;
      const uint32_t j_seq = seq, j_size_a = size_a, j_size_b = size_b;
      const size_t p0 = (size_t)u * unit, cnt = std::min<size_t>(unit, n - p0);
      void (*j_copy)(void*, const void*, size_t) = copy;
      uint32_t (*j_copy_b_form)(void*, const void*, size_t) = copy_b_form;
      // "I have read the job": a finish() that gives up on this thread writes the next job's fields afterwards, and
      // this is the edge that orders those writes behind the reads above (a completed unit orders them through
      // `finished`; a thread that never completes has nothing else to show)
      taken.fetch_add(1, std::memory_order_release);
      j_copy(j_apts + p0 * j_size_a, j_pts + p0 * j_size_a, cnt * j_size_a);
      if (j_size_b && j_copy_b_form)
        __atomic_store_n(j_flags + 16 * (size_t)u + 1, j_copy_b_form(j_acov + p0 * j_size_b, j_cov + p0 * j_size_b, cnt), __ATOMIC_RELAXED);
      else if (j_size_b) j_copy(j_acov + p0 * j_size_b, j_cov + p0 * j_size_b, cnt * j_size_b);
      // the unit's bytes (streaming stores, fenced by `copy`) are globally visible before its flag
      __atomic_store_n(j_flags + 16 * (size_t)u, j_seq, __ATOMIC_RELEASE);
      uint64_t f = finished.load(std::memory_order_relaxed);
      while ((uint32_t)(f >> 32) == my_job &&
             !finished.compare_exchange_weak(f, f + 1, std::memory_order_release, std::memory_order_relaxed)) {}
    }
  }
  void run() {
    uint32_t seen = gen.load(std::memory_order_acquire);
    for (;;) {
      bool have = false;
      for (int spins = 0; spins < 40000 && !have; ++spins) {   // ~1 ms
        have = gen.load(std::memory_order_acquire) != seen;
        if (!have) __builtin_ia32_pause();
        // should the scheduler have put this thread on the CPU of one that has work to do (a wake-up lands on the
        // waker's CPU): let it run.  Costs a fraction of a microsecond when nobody else wants this CPU.
        if (!have && (spins & 1023) == 1023) sched_yield();
      }
      if (!have) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return quit || gen.load(std::memory_order_acquire) != seen; });
        if (quit) return;
      }
      seen = gen.load(std::memory_order_acquire);
      work(seen);
    }
  }
  void start(int helpers) {
    for (int i = 0; i < helpers; ++i) th.emplace_back([this] { run(); });
  }
  // everything of the job is in place: open it (to the helpers too if asked); the caller then works on it itself
  // (work(job)) and waits for the units others took (finish())
  uint32_t post(bool wake_helpers) {
    next_nonzero(job);
    finished.store((uint64_t)job << 32, std::memory_order_relaxed);
    next.store((uint64_t)job << 32, std::memory_order_release);
    if (wake_helpers && !broken && !th.empty()) {
      {
        std::lock_guard<std::mutex> lk(m);
        gen.store(job, std::memory_order_release);
      }
      cv.notify_all();
    }
    return job;
  }
  // Wait for the units other threads took, then CLOSE the job.  A helper that was woken for this job may sit on THIS
  // thread's CPU (a wake-up lands on the waker's CPU) with a unit half copied: spinning here would keep it off the CPU
  // for a whole scheduler slice (3 ms steps were measured); after a short spin the CPU is offered to whoever else wants
  // it.  Bounded: a helper that has not delivered its unit `deadline_seconds` after the caller ran out of work (it died,
  // or the machine is not scheduling it) makes this return false — the job is closed, the crew never wakes a helper
  // again (`broken`), and the caller reports the failure; the late helper's completion is dropped by its job number.
  // (What cannot be taken back is the helper's pointer into the caller's buffer: the entry point says so in its error.)
  bool finish(double deadline_seconds = 10.0) {
    const uint32_t want = units.load(std::memory_order_relaxed);
    bool ok = true;
    double t0 = 0.0;
    for (uint32_t spins = 0; (uint32_t)finished.load(std::memory_order_acquire) < want; ++spins) {
      if (spins < 512) { __builtin_ia32_pause(); continue; }
      sched_yield();
      if ((spins & 255u) == 0) {
        const double t = now_seconds();
        if (t0 == 0.0) t0 = t;
        else if (t - t0 > deadline_seconds) { ok = false; broken = true; (void)taken.load(std::memory_order_acquire); break; }
      }
    }
    next.store(((uint64_t)job << 32) | kClosed, std::memory_order_release);
    if (!ok) finished.store(0, std::memory_order_relaxed);   // job 0 is never posted: late completions go nowhere
    return ok;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
    }
    cv.notify_all();
    for (auto& t : th)
      if (t.joinable()) {
        if (broken) t.detach();   // one of them never came back: nobody may wait for it (the owner leaks this object)
        else t.join();
      }
    th.clear();
  }
};

struct vgicp_multi;  // vgicp_multi.hip: the sub-contexts of an in-process multi-device context

struct vgicp_ctx {
  // FIRST, at offset 0 whatever follows: a mark and this build's sizeof(vgicp_ctx), written by the module that creates the
  // context.  libvgicp_hip_prior.so writes fields of this struct from outside the module and refuses a context whose
  // stamp is not its own build's (vgicp_prior.hip), so a pair from two builds is an error and not a corrupted context.
  static constexpr uint64_t kLayoutMark = 0x7667637000000000ull;   // "vgcp" in the upper half
  uint64_t layout = kLayoutMark | (uint64_t)sizeof(vgicp_ctx);
  uint64_t id = 0;                // creation number (never 0, never reused)
  int device = -1;
  vgicp_multi* multi = nullptr;   // this handle IS a multi-device context: every entry point forwards to vgicp_multi.hip
  vgicp_multi* owner = nullptr;   // this context is one of a multi-device context's sub-contexts (rank = peer_rank)
  // Members are destroyed in reverse order: the stream is declared before every buffer and event, so it outlives
  // everything that may have been enqueued on it.  A new buffer is one member below; nothing else releases it.
  StreamHandle stream;
  mutable std::string err;
  std::string peer_status;   // "" while the device-initiated exchange is wired (or nothing to exchange); else why it is not (vgicp_peer_status)
  int cu_count = 0;
  uint64_t hbm_bytes = 0;
  std::string arch;

  // voxel table
  double voxel_size = 0.0;
  DeviceBuf<VoxelRecord> table;
  uint64_t slots = 0;
  uint64_t voxels = 0;      // FULL records
  uint64_t tombstones = 0;
  DeviceBuf<uint32_t> d_counters;  // 8 words + 64 of developer histograms (VGICP_DEBUG_PREP=2)
  PinnedBuf<uint32_t> h_counters;  // pinned

  // dense copy of the FULL records for tables far beyond the caches' reach (PersistArgs::dense): rebuilt lazily before
  // an align when the map has changed since (map_version counts every mutation)
  DeviceBuf<VoxelRecord> d_dense;
  uint64_t dense_capacity = 0;      // records
  DeviceBuf<uint32_t> d_dense_counts;
  uint32_t dense_counts_capacity = 0;
  uint64_t map_version = 1, dense_version = 0;
  uint64_t dense_slots_threshold = 1ull << 24;   // tables of this many slots (2 GiB) and more; VGICP_DENSE_SLOTS at creation, 0 = never
  // batch staging (upsert / erase / hooks)
  DeviceBuf<void> d_stage;
  DeviceBuf<void> d_cells;  // cell table of the scan preparation (vgicp_preprocess)

  // resident scan
  DeviceBuf<double> d_scan_aos;  // points (3n) then covs (9n)
  DeviceBuf<double> d_scan;      // SoA planes
  DeviceBuf<void> d_memo;        // per point {key, slot}: the launch-per-round loop's memory between launches (IterArgs::memo)
  size_t scan_capacity = 0;      // points
  uint32_t n = 0;
  uint64_t stride = 0;
  bool scan_ready = false;

  // align state
  DeviceBuf<AlignState> d_state;  // two, ping-pong: launch j reads [j&1], writes [(j+1)&1]
  PinnedBuf<AlignState> h_state;  // pinned, kMaxChunksInFlight + 1 slots
  DeviceBuf<double> d_rows[2];    // partial rows, ping-pong like the state
  DeviceBuf<double> d_sums;       // one row: the all-reduce message (multi-GPU)
  // persistent single-launch align (single GPU)
  uint32_t persist_round0 = 0;       // rounds the persistent launches of this context have executed, mod 3
  uint32_t persist_seq = 0;
  uint32_t persist_lds_budget = 0;   // dynamic LDS a persistent workgroup may plan with (0 = the whole CU); sub-contexts that share a device take less
  uint32_t persist_grid = 0;         // workgroups of every persistent launch: min(CUs, kExchangeRows), all resident
  DeviceBuf<double> d_rows_persist;  // [3][kExchangeRows][kSlots] (vgicp_device.h, PersistArgs)
  DeviceBuf<double> d_parts_persist; // [3][kFolders][kSlots]
  PinnedBuf<void> h_exchange_image;  // pinned: what the two buffers hold between launches
  // the batched align (vgicp_hip_batch.h): storage of its own, made with the context
  DeviceBuf<double> d_batch_exchange;  // team rows, then team parts (team_rows_words() + team_parts_words()); all unset before a launch
  PinnedBuf<double> h_batch;           // pinned: VGICP_BATCH_MAX blocks of kBatchSlotRows rows (state, then log), then the abort word's row; .dev(): as the device addresses it
  // scoring poses (vgicp_hip_evaluate.h): storage of its own, made with the context
  DeviceBuf<double> d_eval_rows;       // kEvalRowBudget rows: [poses of a launch][rows per pose][kSlots]
  PinnedBuf<double> h_eval;            // pinned: VGICP_EVAL_MAX result rows of kSlots doubles, then VGICP_EVAL_MAX poses of 12; .dev() likewise
  // the per-point report (vgicp_hip_points.h): storage of its own, made by the first call and grow-only
  DeviceBuf<char> d_points;            // the planes, the keys, the sort's buffers and the counters, for points_capacity points
  size_t points_capacity = 0;          // points (the scan capacity the buffer was sized from)
  PinnedBuf<unsigned long long> h_points;  // pinned, kPointResultWords: the counts and the quantiles; .dev() likewise
  bool persistent_enabled = true;    // cleared by VGICP_PERSISTENT=0 or when a workgroup does not fit a CU
  double prefetch_margin = 0.015;    // see PersistArgs::prefetch_margin; VGICP_PREFETCH_MARGIN overrides (0 = off).  Round 6: 0.03 -> 0.015
                                     // once the workgroups that are no folders stopped polling early (C2: 0 7.18, 0.01 6.41, 0.015 6.34, 0.02 6.35, 0.03 6.52, 0.04 6.66 us per round)
  uint32_t persist_spin_limit = 50000;  // polls (>= ~1 us each) before an in-kernel wait gives up
  int persistent_cooldown = 0;       // aligns left on the per-launch loop after an in-kernel wait timed out
  uint64_t persistent_launches = 0;  // diagnostics (vgicp_get_counter)
  uint64_t persistent_fallbacks = 0;
  uint64_t upload_bytes = 0;
  double upload_seconds = 0.0;
  uint64_t prep_indefinite = 0;      // kept points of the last scan preparation with an indefinite covariance
  bool prep_settled = false;         // h_prep holds the counter block of a preparation that resolve_prepare accepted
  // developer / test switches of the environment, read ONCE when the context is created (never inside a call)
  struct DevSwitches {
    bool no_sym = false, no_stash = false, no_memo = false, verbose = false, insert_sort = false;
    int debug_prep = 0;
    uint32_t pack_spin_limit = 0;     // 0 = the module's default
    long debug_upload_delay_us = 0;
    bool no_fused = false;            // A/B: vgicp_align keeps the pack launch in front of the persistent one
  } dev;
  std::unique_ptr<CopyCrew> crew;    // the upload's copy threads, created with the first upload that wants a helper
  int upload_threads = 3;            // threads that copy a scan into the staging memory, the caller's included (VGICP_UPLOAD_THREADS).
                                     // Round 6: 2 -> 3 — with symmetric covariances crossing the link as six doubles the HOST copy out of
                                     // never-seen pages became the limit at two threads (C2 from fresh clouds: 2 threads 0.366 ms per align
                                     // with or without the compaction, 3 threads 0.321, 4 threads 0.316 - 0.321)
  PinnedBuf<char> h_upload;          // page-locked staging memory of the scan upload: [unit flags][points][covariances]
  size_t upload_cap = 0;             // bytes behind the flags
  size_t upload_flag_bytes = 0;      // one 64-byte line per unit the capacity can hold; never holds anything but flags
  EventHandle ev_upload;             // behind the kernel that read h_upload last (the next upload overwrites it)
  bool upload_in_flight = false;
  uint64_t upload_slow = 0;          // uploads whose copy threads took so long that the packing was repeated behind them
  // scan preparation without host round trips
  DeviceBuf<void> d_tiles;           // tile slots of the two device-wide scans
  PinnedBuf<uint32_t> h_prep;        // pinned: the counter block as a preparation left it (kCounterWords)
  uint32_t prep_epoch = 0;
  bool scan_pending = false;         // a prepared scan is resident but the host has not read its size / verdict yet
  uint32_t n_upper = 0;              // raw points of the pending scan (>= its kept points)
  uint64_t scan_generation = 0;      // replacements of the resident scan so far (VGICP_COUNTER_SCAN_GENERATION)
  uint32_t scan_seq = 0;             // uploads so far; pack_scan_kernel marks an asymmetric covariance with it
  bool scan_sym_known = false;       // the resident scan went through pack_scan_kernel (not a scan prepared on the device)
  int64_t prep_deskewed = 0;
  // what vgicp_scan_info answers for the RESIDENT scan: its own preparation's counts, taken when that is settled.  prep_deskewed
  // and prep_indefinite are the LAST preparation's, vgicp_preprocess included, which leaves the resident scan alone
  int64_t scan_deskewed = 0;
  uint64_t scan_indefinite = 0;
  // the robust round (include/vgicp_hip_robust.h), as vgicp_set_option left it; kernel 0 and gate 0 = the plain round
  int robust_kernel = 0;             // VGICP_OPTION_ROBUST_KERNEL
  int robust_scale_micro = 1000000;  // VGICP_OPTION_ROBUST_SCALE_MICRO: c = value / 1e6
  int robust_gate_micro = 0;         // VGICP_OPTION_GATE_MICRO: gate on d^2 = value / 1e6, 0 = none
  // the pose prior (include/vgicp_hip_prior.h), as vgicp_set_pose_prior left it
  bool prior_on = false;
  double prior_pose[12] = {0};       // R0 column-major (9) then t0 (3)
  double prior_info[21] = {0};       // lower triangle, row by row
  bool reference_order = false;      // VGICP_OPTION_REFERENCE_ORDER: prepared scans come in the reference's unordered_map order
  bool prep_with_deskew = false;
  double prep_voxel = 0.0;           // > 0: the resident scan was down-sampled on the device to one point per voxel of this size
  // the deskew's state table on its way to the device: pinned, two slots in turn (an enqueue-only preparation returns
  // before the copy has run, so the table cannot live on the caller's stack)
  // ... and the raw sweep (points, then capture times): mid-sized copies out of the caller's pageable memory are staged
  // through these instead of handed to the runtime, which would pin the caller's pages on the fly — measured on the
  // round's boxes: 1.4 MB of points 0.05 ms staged, but 12-22 ms (first copy of every frame) through the pinning path
  // once the caller allocates and frees its clouds per frame, as the reference does (examples/frame_chain)
  // ... and for every OTHER copy between the caller's pageable memory and the device (map batches, hooks, scan_download,
  // the scan of a vgicp_align up to 4 MB): one page-locked arena.  A copy of more than 512 KB goes through it (h2d: CPU
  // copy in, then DMA; d2h: DMA, then CPU copy out after the call's synchronisation) -- never through the runtime's
  // pin-on-the-fly path, whose registrations stall the whole process when the caller frees the buffer
  PinnedBuf<char> h_arena;
  size_t arena_used = 0;
  size_t upload_stage_limit = 512u << 20;   // scans up to this many bytes are staged by the copy crew; larger ones (and
                                            // all of them with the limit 0) are handed to the runtime in place
                                            // (VGICP_UPLOAD_STAGE_LIMIT, VGICP_OPTION_UPLOAD_STAGE_KB)
  size_t upload_whole_hint = 0;             // a sub-context's shard: the size of the caller's WHOLE scan decides, not the shard's
  struct PendingOut { void* dst; const char* src; size_t bytes; };
  std::vector<PendingOut> pending_out;
  // vgicp_scan_fetch_*: the prepared scan written into page-locked memory by a kernel, piece by piece
  PinnedBuf<unsigned long long> h_fetch_hdr;      // pinned: word 0 epoch << 32 | kept (run_scan_kernel), word 8 seq << 32 | refused (fetch_kernel), words 16 .. 79 the checksums
  PinnedBuf<char> h_fetch;           // pinned: [one 64-byte flag line per piece][points, padded to 256 bytes][covariances]
  size_t fetch_cap_points = 0;       // points the staging area can hold
  size_t fetch_flag_bytes = 0;
  uint32_t fetch_seq = 0;
  DeviceBuf<unsigned long long> d_fetch_sums;   // device, 65 words, zero between launches (fetch_kernel's checksums + ticket)
  bool fetch_sums_valid = false;     // the page-locked copy (h_fetch_hdr + 16 .. + 80) holds the sums of the last completed fetch
  bool fetch_open = false;           // a fetch kernel is enqueued behind the pending preparation
  uint32_t fetch_kept = 0;
  // sweeps staged AHEAD of their preparation (vgicp_sweep_stage: the lidar callback's thread copies a sweep into
  // page-locked memory when it arrives; vgicp_scan_prepare_staged_async consumes it by ticket).  Guarded by
  // ahead_mutex: the one part of a context that another thread may enter while the owner thread is inside a call.
  struct AheadSlot {
    PinnedBuf<char> mem;
    size_t cap = 0, n = 0;
    uint64_t ticket = 0;
    bool has_times = false;
    uint32_t step = 0, off[3] = {0, 0, 0};   // != 0: sensor records (vgicp_sweep_stage_cloud2), float32 x y z at these offsets
    size_t times_at = 0;           // byte offset of the capture times (n doubles) inside mem
    int state = 0;                 // 0 free, 1 staged, 2 handed to the device (`done` recorded behind its readers), 3 being filled,
                                   // 4 being handed to the device (vgicp_scan_prepare_staged_async is enqueuing its readers)
    EventHandle done;
  };
  AheadSlot ahead[3];
  std::mutex ahead_mutex;
  uint64_t ahead_tickets = 0;
  PinnedBuf<char> h_raw_stage[2];
  size_t raw_stage_cap[2] = {0, 0};
  PinnedBuf<double> h_state_table[2];
  size_t state_table_cap[2] = {0, 0};
  EventHandle ev_state_table[2];
  uint32_t state_table_next = 0;
  // deferred map insertion (vgicp_map_insert_resident_async): running totals on the device, read at the next sync
  uint32_t* d_ins_counters = nullptr;  // not owned: d_counters + kCounterWords
  PinnedBuf<uint32_t> h_ins_counters;  // pinned
  uint32_t ins_seen[2] = {0, 0};
  bool insert_pending = false;
  bool ins_copy_enqueued = false;    // some device-to-host copy behind the pending insertion carries its totals ...
  bool ins_from_prep = false;        // ... in the tail of h_prep (the next preparation's counter copy) rather than h_ins_counters
  uint64_t insert_pending_upper = 0;
  // gated insertion (include/vgicp_hip_map_gated.h): the decision's running totals on the device (d_ins_counters +
  // kGateWord), what the host has read of them, and the totals since vgicp_map_reset
  uint32_t gate_seen[3] = {0, 0, 0};
  bool gate_pending = false;         // the pending insertion is a gated one: its totals travel with the insertion's
  uint64_t gated_points = 0, gated_refused = 0;
  // free-space carving (include/vgicp_hip_map_carve.h).  A deferred carve's counts are running totals on the device
  // (d_ins_counters + kCarveRaysWord / kCarveRemovedWord); the synchronisation that settles reads them with the
  // insertion's and applies voxels -= removed, tombstones += removed.  A removal leaves voxels + tombstones, the sum
  // plan_table_growth plans with, as it is: a pending carve needs no upper bound in the growth plan (unlike
  // insert_pending_upper), and by itself it makes no deferred call wait
  bool carve_pending = false;
  uint32_t carve_seen[2] = {0, 0};   // rays, removed: what the host has read of the running totals
  uint64_t carve_rays = 0, carve_removed = 0;   // since vgicp_map_reset
  PinnedBuf<int32_t> h_carve_keys;   // pinned, grow-only: the synchronous call's key list on its way to the caller
  size_t carve_keys_capacity = 0;    // voxels
  // the ray report (include/vgicp_hip_map_rays.h): read-only, so what it confirms lives beside the table
  DeviceBuf<uint32_t> d_ray_bits;    // one bit per slot and pose of a group (ray_group_poses, vgicp_map_plan.h); made by the
                                     // first call, anew only when the table's slot count has changed
  uint64_t ray_bits_slots = 0;       // the slot count d_ray_bits was sized for
  PinnedBuf<char> h_rays;            // pinned, grow-only: the poses on their way in, the counts and the planes on their way out
  // the map's coarser levels (include/vgicp_hip_map_levels.h): nothing of this is allocated while levels_requested == 0.
  // level[l - 1] is level l: an open-addressing table like the map's, never with a dense copy; version: the map_version
  // it was built at (0: never, or emptied), checked by every call that reads a level (ensure_levels, as ensure_dense)
  struct MapLevel {
    DeviceBuf<VoxelRecord> table;
    uint64_t slots = 0;
    uint64_t voxels = 0;             // known once level_counts_pending is false
    uint64_t version = 0;
  };
  int levels_requested = 0;
  MapLevel level[VGICP_LEVELS_MAX];
  DeviceBuf<uint32_t> d_level_counts;    // per level {voxels, probe sequences exhausted}
  PinnedBuf<uint32_t> h_level_counts;    // pinned: the same, copied behind every rebuild
  bool level_counts_pending = false;     // that copy is enqueued and nobody has waited for it yet
  int view_level = 0;                    // != 0 only inside a stage of vgicp_align_resident_levels: resident_view() is that level's
  // locate (include/vgicp_hip_map_locate.h): read-only, storage of its own and of one size (LocateLayout,
  // vgicp_capi_map_locate.inl), made by the first call
  DeviceBuf<char> d_locate;              // the poses, the skipped points per pose, the plane of hits
  PinnedBuf<char> h_locate;              // pinned: the poses on their way in, the bests (.dev(): where the best launch writes them), the plane on its way out
  // submap as scan (include/vgicp_hip_map_submap.h), as the DESTINATION of vgicp_scan_from_map; made by the first call,
  // grow-only
  DeviceBuf<char> d_submap_work;         // the call's scratch (submap_work_bytes): ballots, the groups' counts, the totals
  DeviceBuf<char> d_submap_keys;         // per point of the scan: the counts (8 bytes each), then the keys (12 bytes each)
  size_t submap_capacity = 0;            // points d_submap_keys holds
  PinnedBuf<unsigned long long> h_submap;   // pinned, 4 words; .dev(): where the scan launch writes the totals
  uint64_t submap_generation = 0;        // the scan_generation vgicp_scan_from_map left (0: it never ran): the keys are that scan's
  EventHandle ev_submap;                 // as the SOURCE of a call between two contexts: behind this stream's work, for dst's stream to wait on
  // the map checkpoint (include/vgicp_hip_map_checkpoint.h); made by the first call, grow-only.  The device side of a
  // call is carved out of the staging area (d_stage)
  PinnedBuf<char> h_checkpoint;          // pinned: the blob on its way out (header room, then the payload) or in
  size_t checkpoint_capacity = 0;        // bytes h_checkpoint holds
  PinnedBuf<unsigned long long> h_checkpoint_totals;   // pinned, 4 words; .dev(): where the scan launch writes {FULL, TOMB, raw points}
  // map merge (include/vgicp_hip_map_merge.h), as the DESTINATION of vgicp_map_merge; made by the first call.  The device
  // side of a call is carved out of the staging area (d_stage); as the SOURCE a context lends ev_submap
  PinnedBuf<unsigned long long> h_merge;   // pinned, kMergeTotalWords; .dev(): where the scan launch writes {selected, too far, too few}
  // raw points of the map (VGICP_OPTION_MAP_RAW_POINTS): the device append log of vgicp_device.h's RawLog.  Its three
  // device words sit behind the insertion's totals (d_ins_counters + 4), so the copy that brings those to the host in
  // the frame chain brings the log's fill too: the bound below is made exact at every synchronisation that settles an
  // insertion, and the log grows (one synchronisation) only when it could fill
  bool raw_on = false;
  DeviceBuf<RawPoint> d_raw;
  uint32_t raw_capacity = 0;         // entries
  uint64_t raw_used_upper = 0;       // entries appended so far, at most
  size_t raw_hint = 0;               // the last vgicp_map_reset's capacity_hint
  bool raw_broken = false;           // an append did not fit: the store refuses every call until it is made anew
  PinnedBuf<uint32_t> h_raw_ctr;     // pinned, 4 words: the log's device words after a synchronous call
  // frame statistics
  uint64_t stat_launches0 = 0, stat_copies0 = 0, stat_syncs0 = 0;
  bool stage_events = false;
  EventHandle ev_stage[7];  // [6]: behind the prologue
  bool ev_stage_set[7] = {false, false, false, false, false, false, false};
  int iter_block = 512;           // threads per workgroup of the iteration kernel (measured best at C2)
  // the log: each block begins with ONE HEADER ROW (the persistent launch leaves its final AlignState there, so a single
  // device-to-host copy brings state and log back); the iterations' rows follow it
  DeviceBuf<double> d_log;
  PinnedBuf<double> h_log;  // .dev(): the same memory as the device addresses it (the persistent launch writes state + log there)
  double* d_log_rows() const { return d_log + kSlots; }
  double* h_log_rows() const { return h_log + kSlots; }
  double* h_log_rows_dev() const { return h_log.dev() + kSlots; }
  int log_capacity = 0;     // iterations
  DeviceBuf<uint64_t> d_stamps;  // only with VGICP_DEBUG_STAMPS=1
  DeviceBuf<unsigned long long> d_unit_clock;  // FusedUpload::unit_clock
  double wall_clock_hz = 0.0;    // the device's constant clock (s_memrealtime)
  EventHandle ev_begin, ev_end;
  EventHandle ev_chunk[kMaxChunksInFlight];
  std::vector<EventHandle> ev_prof;

  // device-initiated exchange between GPUs: peer-mapped mailboxes (vgicp_peer_*)
  DeviceBuf<double> d_mail;            // this rank's mailbox, fine-grained device memory, [3][kMaxRanks][kSlots]
  double* peer_mail[kMaxRanks] = {nullptr};  // every rank's mailbox as mapped here ([peer_rank] = d_mail).  Not owned: IPC
                                       // mappings that close_peers closes, or plain pointers of sibling contexts
  DeviceBuf<double*> d_mail_table;     // device copy of peer_mail
  int peer_world = 1, peer_rank = 0;
  bool peers_connected = false;
  bool peer_mail_is_ipc = true;        // false: plain pointers of the same process (sub-contexts), nothing to close
  bool peer_enabled = true;            // cleared for good when a launch gave up waiting for a peer
  uint32_t mail_round0 = 0;            // rounds executed through the mailboxes so far (same on every rank)
  uint32_t mail_seq = 0;               // aligns attempted through the mailboxes so far (same on every rank)

  // RCCL
  RcclApi rccl;
  ncclComm_t comm = nullptr;
  int world_size = 1;
  int rank = 0;
};

// The facts plan_align (vgicp_align_plan.h) decides by, as this context and this call have them: the ONE place where a
// single-device align's plan meets the context (a multi-device context fills its own: group_facts, vgicp_multi.hip).
// n: the caller's count (AlignCall::Upload), else the resident scan's.
inline AlignFacts call_facts(AlignCall call, uint32_t flags, int max_iteration) {
  AlignFacts f;
  f.call = call;
  f.max_iteration = max_iteration;
  f.profile = (flags & VGICP_FLAG_PROFILE) != 0;
  f.no_persistent = (flags & VGICP_FLAG_NO_PERSISTENT) != 0;
  return f;
}
inline bool robust_on(const vgicp_ctx* ctx) { return ctx->robust_kernel != 0 || ctx->robust_gate_micro != 0; }
// The resident scan and the voxel map as a launch sees them: the ONE place where an argument struct's view is filled.
inline vgicp::ResidentView resident_view(const vgicp_ctx* ctx) {
  if (ctx->view_level != 0) {   // a stage of vgicp_align_resident_levels: the level is just another (table, mask, voxel_size)
    const vgicp_ctx::MapLevel& l = ctx->level[ctx->view_level - 1];
    return vgicp::ResidentView{ctx->d_scan, ctx->stride, ctx->n, (uint32_t)(l.slots - 1), l.table,
                               level_voxel_size(ctx->voxel_size, ctx->view_level)};
  }
  return vgicp::ResidentView{ctx->d_scan, ctx->stride, ctx->n, (uint32_t)(ctx->slots - 1), ctx->table, ctx->voxel_size};
}
// What a launch's asym_dev is (with scan_seq = ctx->scan_seq): word 2 of the insertion's counter block, the symmetry
// verdict of pack_scan_kernel, for a scan that went through it (developer A/B no_sym: always read all twelve planes).
inline const uint32_t* symmetry_word(const vgicp_ctx* ctx) {
  return (ctx->scan_sym_known && !ctx->dev.no_sym) ? ctx->d_ins_counters + 2 : nullptr;
}
template <class Args> void set_symmetry(const vgicp_ctx* ctx, Args* a) {   // the pair, wherever an argument struct keeps it
  a->asym_dev = symmetry_word(ctx);
  a->scan_seq = ctx->scan_seq;
}
// The context's robust settings and its pose prior as the kernels take them.
inline vgicp::RobustArgs robust_args(const vgicp_ctx* ctx) {
  const double c = (double)ctx->robust_scale_micro / 1000000.0;
  return vgicp::RobustArgs{(uint32_t)ctx->robust_kernel, c * c, (double)ctx->robust_gate_micro / 1000000.0};
}
inline vgicp::PriorArgs prior_args(const vgicp_ctx* ctx) {
  vgicp::PriorArgs p;
  p.on = 1u;
  for (int k = 0; k < 12; ++k) p.pose[k] = ctx->prior_pose[k];
  for (int k = 0; k < 21; ++k) p.info[k] = ctx->prior_info[k];
  return p;
}
inline AlignFacts align_facts(const vgicp_ctx* ctx, const vgicp_params* params, AlignCall call, uint64_t n, size_t k = 1) {
  AlignFacts f = call_facts(call, params ? params->flags : 0u, params ? params->max_iteration : 0);
  f.n = n;
  f.k = k;
  f.persistent_enabled = ctx->persistent_enabled;
  f.owner = ctx->owner != nullptr;
  f.comm = ctx->comm != nullptr;
  f.peers_connected = ctx->peers_connected;
  f.peer_enabled = ctx->peer_enabled;
  f.stamps = ctx->d_stamps != nullptr;
  f.stage_events = ctx->stage_events;
  f.no_fused = ctx->dev.no_fused;
  f.world_size = ctx->world_size;
  f.peer_world = ctx->peer_world;
  f.cooldown = ctx->persistent_cooldown;
  f.grid = ctx->persist_grid;
  f.robust = robust_on(ctx);
  f.prior = ctx->prior_on;
  return f;
}

// ---- helpers shared by the two translation units ----
namespace vgicp {
inline int fail(const vgicp_ctx* ctx, int code, const std::string& text) {
  if (ctx) {
    ctx->err = text;
    if (g_stage_error_ctx == ctx->id) g_stage_error_ctx = 0;
  } else {
    g_create_error = text;
  }
  return code;
}
inline int fail_stage(const vgicp_ctx* ctx, int code, const std::string& text) {
  g_stage_error = text;
  g_stage_error_ctx = ctx ? ctx->id : 0;
  return code;
}
inline int fail_hip(const vgicp_ctx* ctx, hipError_t e, const char* what) {
  return fail(ctx, VGICP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace vgicp

#define VG_HIP(ctx, call)                                              \
  do {                                                                 \
    hipError_t e__ = (call);                                           \
    if (e__ != hipSuccess) return fail_hip((ctx), e__, #call);         \
  } while (0)
// ... and a call of this library's own that returns a status: anything but VGICP_OK is returned as it is
#define VG_RC(call) do { const int rc__ = (call); if (rc__ != VGICP_OK) return rc__; } while (0)

// The layout handshake of the libraries beside the module (vgicp_<name>.hip for every name of the Makefile's SIDE): was
// this context made by the build that reads it?  Reads the stamp only.
inline bool same_build(const vgicp_ctx* ctx) { return ctx->layout == (vgicp_ctx::kLayoutMark | (uint64_t)sizeof(vgicp_ctx)); }
// ... as every entry point of those libraries makes it, under VG_RC, before anything else of the context is read or
// written: a NULL context leaves no text, one of another build leaves `refusal` (the library's own words) where a failed
// vgicp_create's text goes (vgicp_last_error(NULL)).
inline int layout_handshake(const vgicp_ctx* ctx, const char* refusal) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  return same_build(ctx) ? VGICP_OK : vgicp::fail(nullptr, VGICP_ERR_BAD_ARGUMENT, refusal);
}

// ---- what vgicp_multi.hip needs from vgicp_capi.hip besides the public entry points ----
namespace vgicp_internal {
// A sub-context gives up an align it cannot finish alone with this status (never seen by a caller of the ABI): the
// in-kernel exchange between the sub-contexts timed out, or the align asks for the launch-per-round loop — the
// multi-device context then runs that loop itself, adding the sub-contexts' rows on the host.
constexpr int kNeedGroupLoop = 1000;
// vgicp_create with a cap on the persistent launch's workgroups (sub-contexts that share one device split its CUs).
int create_context(int device_id, uint32_t max_persist_grid, vgicp_ctx** out);
// Mailboxes of the device-initiated exchange wired by plain pointers (one process: no IPC handles); (re-)initialises
// every mailbox and the running round / align numbers.  The streams of all sub-contexts must be idle.
int wire_mailboxes(vgicp_ctx* const* subs, int n);
// ICP::align over sub-contexts that each hold a shard, one launch per round on every device, the rank rows added on
// the host in rank order (the same pairwise tree the mailbox path uses): the fallback of the in-kernel exchange and
// the path of VGICP_FLAG_PROFILE / VGICP_FLAG_NO_PERSISTENT.  The caller's thread drives every device.
int align_host_summed(vgicp_ctx* const* subs, int n, const double guess[16], const vgicp_params* params,
                      double out_pose[16], vgicp_stats* stats);
// The resident scan of `ctx` becomes n points that are already on a device as AoS (points n x 3, covs n x 9; peer
// memory is fine): copied into the context's own storage and packed into the planes the registration reads.
// Enqueued on the context's stream (which first waits for `ready`, if given); not synchronised.
int adopt_device_scan(vgicp_ctx* ctx, int src_device, const double* d_points, const double* d_covs, size_t n,
                      double prep_voxel, hipEvent_t ready);
// LocalMap::updateLocalMap's insertion for n points that are already on THIS context's device as AoS.
int map_insert_device(vgicp_ctx* ctx, const double* d_points, const double* d_covs, size_t n, const double transform[16],
                      size_t max_points_per_voxel, bool short_lists, bool deferred, size_t* new_voxels);
int settle_context(vgicp_ctx* ctx);
// vgicp_align_resident_batch as k single aligns in a row (vgicp_capi_batch.inl); *first_bad: the first hypothesis status
// that is not VGICP_OK
int align_batch_sequential(vgicp_ctx* ctx, size_t k, const double* guesses, const vgicp_params* params, double* out_poses,
                           vgicp_batch_stats* stats, bool loop_only, int* first_bad);
// vgicp_points_resident (include/vgicp_hip_points.h) behind its entry point in libvgicp_hip_points.so, which has made
// the layout handshake: every other check, the settling, the launches, the delivery (vgicp_capi_points.inl).
int points_resident(vgicp_ctx* ctx, const double pose[16], size_t capacity, double* d2, double* sq_error, double* weight,
                    uint8_t* status, size_t n_quantiles, const double* q, vgicp_point_summary* summary,
                    vgicp_point_stats* stats);
// The entry points of include/vgicp_hip_map_gated.h behind libvgicp_hip_map_gated.so, which has made the handshake
// (vgicp_capi_map_gated.inl).
int map_insert_resident_gated(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, double gate,
                              size_t capacity, uint8_t* kept, vgicp_gated_insert_stats* stats);
int map_insert_resident_gated_async(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, double gate);
int map_gated_totals(vgicp_ctx* ctx, uint64_t* points, uint64_t* refused);
// The entry points of include/vgicp_hip_map_carve.h behind libvgicp_hip_map_carve.so, likewise (vgicp_capi_map_carve.inl).
int map_carve_resident(vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params* params, size_t capacity,
                       int32_t* removed_keys, size_t* removed, vgicp_carve_stats* stats);
int map_carve_resident_async(vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params* params);
int map_carve_totals(vgicp_ctx* ctx, uint64_t* rays, uint64_t* removed);
// The entry point of include/vgicp_hip_map_rays.h behind libvgicp_hip_map_rays.so, likewise (vgicp_capi_map_rays.inl).
int rays_resident(vgicp_ctx* ctx, const double* poses, size_t n_poses, const vgicp_ray_params* params,
                  const vgicp_ray_outputs* per_point, vgicp_ray_counts* counts, vgicp_ray_stats* stats);
// The entry point of include/vgicp_hip_search_report.h behind libvgicp_hip_search_report.so, likewise (vgicp_capi_prepare.inl).
int prepare_search_report(vgicp_ctx* ctx, vgicp_search_report* report);
// The entry points of include/vgicp_hip_map_levels.h behind libvgicp_hip_map_levels.so, likewise (vgicp_capi_map_levels.inl).
int map_levels_build(vgicp_ctx* ctx, int levels, vgicp_levels_stats* stats);
int map_level_size(vgicp_ctx* ctx, int level, size_t* voxels, size_t* table_slots, double* voxel_size);
int map_level_export(vgicp_ctx* ctx, int level, size_t capacity, int32_t* keys, double* means, double* covs, uint64_t* counts,
                     size_t* written);
int align_resident_levels(vgicp_ctx* ctx, const double guess[16], size_t stages, const int32_t* levels, const vgicp_params* params,
                          double out_pose[16], vgicp_stats* stats);
// The entry point of include/vgicp_hip_map_locate.h behind libvgicp_hip_map_locate.so, likewise (vgicp_capi_map_locate.inl).
int locate_resident(vgicp_ctx* ctx, const double* poses, size_t k, const vgicp_locate_params* params, vgicp_locate_best* best,
                    uint32_t* hits, vgicp_locate_stats* stats);
// The entry points of include/vgicp_hip_map_submap.h behind libvgicp_hip_map_submap.so, likewise (vgicp_capi_map_submap.inl).
int scan_from_map(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_submap_params* params, vgicp_submap_stats* stats);
int scan_from_map_keys(vgicp_ctx* dst, size_t capacity, int32_t* keys, uint64_t* counts, size_t* written);
// The entry points of include/vgicp_hip_map_checkpoint.h behind libvgicp_hip_map_checkpoint.so, likewise
// (vgicp_capi_map_checkpoint.inl); vgicp_map_checkpoint_info needs no context and stays in its library.
int map_checkpoint_size(vgicp_ctx* ctx, size_t* bytes);
int map_checkpoint(vgicp_ctx* ctx, size_t capacity, void* blob, size_t* written, vgicp_checkpoint_stats* stats);
int map_restore(vgicp_ctx* ctx, const void* blob, size_t bytes, vgicp_checkpoint_stats* stats);
// The entry point of include/vgicp_hip_map_merge.h behind libvgicp_hip_map_merge.so, likewise (vgicp_capi_map_merge.inl).
int map_merge(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_merge_params* params, vgicp_merge_stats* stats);
bool align_needs_allocation(const vgicp_ctx* ctx, size_t n, int max_it);
int reserve_for_align(vgicp_ctx* ctx, size_t n, int max_it);
}  // namespace vgicp_internal

// ---- vgicp_multi.hip: the entry points of a multi-device context (ctx->multi != nullptr) ----
namespace vgicp_multi_api {
int destroy(vgicp_ctx* ctx);
int device_info(const vgicp_ctx* ctx, char* name, size_t name_len, int32_t* cu_count, uint64_t* hbm_bytes);
int get_counter(const vgicp_ctx* ctx, int which, uint64_t* value);
int map_reset(vgicp_ctx* ctx, double voxel_size, size_t capacity_hint);
int map_upsert(vgicp_ctx* ctx, size_t n, const int32_t* keys, const double* means, const double* covs);
int map_erase(vgicp_ctx* ctx, size_t n, const int32_t* keys);
int map_size(const vgicp_ctx* ctx, size_t* voxels, size_t* table_slots);
int map_insert_scan(vgicp_ctx* ctx, size_t n, const double* points, const double* covs, const double transform[16],
                    size_t max_points_per_voxel, size_t* new_voxels);
int map_insert_resident(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, size_t* new_voxels,
                        bool deferred);
int map_evict(vgicp_ctx* ctx, const double position[3], double distance_threshold, size_t* removed);
int map_export(vgicp_ctx* ctx, size_t capacity, int32_t* keys, double* means, double* covs, uint64_t* counts,
               size_t* written);
int align(vgicp_ctx* ctx, size_t n, const double* points, const double* covs, const double guess[16],
          const vgicp_params* params, double out_pose[16], vgicp_stats* stats);
int scan_upload(vgicp_ctx* ctx, size_t n, const double* points, const double* covs);
int align_resident(vgicp_ctx* ctx, const double guess[16], const vgicp_params* params, double out_pose[16],
                   vgicp_stats* stats);
int align_resident_batch(vgicp_ctx* ctx, size_t k, const double* guesses, const vgicp_params* params, double* out_poses,
                         vgicp_batch_stats* stats, int* first_bad);
int align_batch_width(vgicp_ctx* ctx, size_t* hypotheses_per_launch);
int scan_prepare(vgicp_ctx* ctx, size_t n, const double* points, const double* point_time, size_t num_states,
                 const double* states, const double extrinsic[16], double voxel_size, int knn, size_t* kept,
                 int64_t* deskewed, bool deferred, uint64_t ticket = 0);
int scan_info(vgicp_ctx* ctx, size_t* kept, int64_t* deskewed, uint64_t* indefinite);
int scan_download(vgicp_ctx* ctx, size_t capacity, double* points, double* covs, size_t* n);
int get_frame_stats(vgicp_ctx* ctx, vgicp_frame_stats* out, int reset);
int set_option(vgicp_ctx* ctx, int option, int value);
vgicp_ctx* first(const vgicp_ctx* ctx);  // sub-context 0: the hooks that work on one device
const char* peer_status(const vgicp_ctx* ctx);
void scan_replaced(vgicp_ctx* ctx);
}  // namespace vgicp_multi_api
