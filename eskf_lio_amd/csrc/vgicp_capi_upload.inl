// vgicp_capi_upload.inl — part of vgicp_capi.hip.
// The scan upload of vgicp_align / vgicp_scan_upload: the copy crew, the staging memory, pack_arena_kernel's launch;
// vgicp_host_register.
extern "C" {

namespace {
// Copy the scan to the device and pack it into the SoA planes (reference: the deep copy of the cloud at
// src/Registration.cpp:11, which here is the copy to the device).  The caller's buffers are ordinary pageable memory
// (std::vector storage) that the caller may free on return, as the reference frees its cloud every frame
// (src/Odometry.cpp:84-87) — so the runtime must never get to register them (a freed registered range takes every
// queue of the process off the device for ~20 ms).  The copy crew (vgicp_context.h) moves the scan into page-locked
// staging memory of the context, this thread and `upload_threads - 1` helpers, unit by unit, while ONE kernel launch
// reads the staged units over PCIe behind them and packs them: 9.6 MB in 0.19 - 0.20 ms, the link's rate, where the
// runtime's in-place path took 0.27 - 0.6 ms and staging with copy commands 0.45 - 0.68 ms.  The pack kernel (and whatever
// the caller enqueues next) runs in stream order; nothing on the DEVICE is waited for here, but the copy threads are:
// the caller's buffers are free again on return.
// Page-locked buffers (vgicp_host_register, hipHostMalloc) are read by the copy engine in place.  In place as well,
// through the runtime's pin-on-the-fly path: scans larger than the stage limit (default 512 MB) and every scan with
// the limit 0 (VGICP_OPTION_UPLOAD_STAGE_KB / VGICP_UPLOAD_STAGE_LIMIT / VGICP_STAGE_LIMIT=0) — for callers that keep
// their buffers.
constexpr uint32_t kPackSpinLimit = 400000;   // polls of a staged unit's flag (>= 1 us each) before the pack kernel gives up
constexpr double kCrewSlowSeconds = 0.1;      // copy threads slower than this: the packing is repeated behind the launch

// CopyCrew::finish() ran into its deadline: a helper thread took a unit of the upload and never delivered it.  The kernel
// that waits for that unit's flag gives up by itself (kPackSpinLimit); the scan is not resident; the context copies
// alone from now on.  The one thing that cannot be taken back is that helper's pointer into the caller's buffer.
int crew_gave_up(vgicp_ctx* ctx) {
  ctx->scan_ready = false;
  ctx->upload_threads = 1;
  (void)hipStreamSynchronize(ctx->stream);
  // that thread may still write the staging memory it was copying into: it is given up (leaked), later uploads get
  // memory of their own
  (void)ctx->h_upload.release();
  ctx->upload_cap = ctx->upload_flag_bytes = 0;
  for (int k = 0; k < 2; ++k) { (void)ctx->h_raw_stage[k].release(); ctx->raw_stage_cap[k] = 0; }
  return fail(ctx, VGICP_ERR_TIMEOUT,
              "a copy thread of the scan upload did not deliver its unit within 10 s (dead or never scheduled): the scan is "
              "not resident, this context stages alone from now on; that thread may still read the caller's buffer");
}

int ensure_upload_stage(vgicp_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->upload_cap) return VGICP_OK;
  if (ctx->upload_in_flight) { VG_HIP(ctx, hipEventSynchronize(ctx->ev_upload)); ctx->upload_in_flight = false; }
  const size_t want = std::max<size_t>(bytes + bytes / 4, 4u << 20);
  const size_t flag_bytes = (want / ((size_t)pack_arena_unit() * kScanPlanes * sizeof(double)) + 2) * 64;
  // the flag area: "no upload yet" (a sequence number is never 0)
  VG_RC(grow_pinned(ctx, &ctx->h_upload, &ctx->upload_cap, flag_bytes + want, flag_bytes));
  ctx->upload_cap = want;
  ctx->upload_flag_bytes = flag_bytes;
  return VGICP_OK;
}

// Whether scan_upload_enqueue stages this scan through the copy threads (else the runtime copies it in place).
bool upload_is_staged(const vgicp_ctx* ctx, size_t n, const double* points, const double* covs) {
  const size_t bytes = n * kScanPlanes * sizeof(double);
  const size_t whole_bytes = ctx->upload_whole_hint ? ctx->upload_whole_hint : bytes;
  return !staging_off() && whole_bytes <= ctx->upload_stage_limit && bytes > (256u << 10) &&
         !(is_pagelocked(points) && is_pagelocked(covs));
}

// One job of the copy crew: n points of the caller's array a (and b, if any) into page-locked staging memory, unit by
// unit (pack_arena_unit() points), every unit published through its flag line under `seq`.
struct CopyJob {
  const void *src_a = nullptr, *src_b = nullptr;
  char *dst_a = nullptr, *dst_b = nullptr;
  uint32_t size_a = 0, size_b = 0;   // bytes per point (size_b = 0: one array only)
  uint32_t (*copy_b_form)(void*, const void*, size_t) = nullptr;   // CopyCrew::copy_b_form
  uint32_t* flags = nullptr;
  size_t n = 0;
  uint32_t seq = 0;
  size_t bytes = 0, wake_bytes = 0;  // the helpers are woken (started) for jobs of wake_bytes and more
  bool helpers = false;              // from here on: set by crew_post
  uint32_t ticket = 0;
  double t_post = 0.0;
};

// The copy threads start on the job: the helpers (if any are awake or worth waking) at once, the caller joins through
// crew_join when it has launched the kernel that reads the staging memory.
void crew_post(vgicp_ctx* ctx, CopyJob* job) {
  const uint32_t unit = pack_arena_unit();
  job->helpers = ctx->upload_threads > 1 && job->bytes >= job->wake_bytes;
  if (!ctx->crew) ctx->crew.reset(new CopyCrew);
  CopyCrew* crew = ctx->crew.get();
  if (job->helpers && crew->th.empty()) crew->start(ctx->upload_threads - 1);
  crew->pts = static_cast<const char*>(job->src_a);
  crew->cov = static_cast<const char*>(job->src_b);
  crew->apts = job->dst_a;
  crew->acov = job->dst_b;
  crew->flags = job->flags;
  crew->n = (uint32_t)job->n;
  crew->unit = unit;
  crew->units = (uint32_t)((job->n + unit - 1) / unit);
  crew->seq = job->seq;
  crew->size_a = job->size_a;
  crew->size_b = job->size_b;
  crew->copy = stage_copy;
  crew->copy_b_form = job->copy_b_form;
  job->t_post = now_seconds();
  job->ticket = crew->post(job->helpers);
}

// This thread copies too, then waits for the helpers: the caller's buffers are free again on return.  *slow: the copy
// threads were held up for so long (kCrewSlowSeconds) that a kernel waiting for their units may have stopped waiting —
// counted here, once.  A helper that never delivers ends the upload (crew_gave_up).
int crew_join(vgicp_ctx* ctx, const CopyJob& job, bool* slow) {
  *slow = false;
  // test aid: a copy thread that is held up
  const long debug_delay_us = ctx->dev.debug_upload_delay_us;
  if (debug_delay_us > 0 && !job.helpers) std::this_thread::sleep_for(std::chrono::microseconds(debug_delay_us));
  ctx->crew->work(job.ticket);
  if (!ctx->crew->finish()) return crew_gave_up(ctx);   // always: the caller's buffers must not be in use on return
  if (now_seconds() - job.t_post > kCrewSlowSeconds) {
    *slow = true;
    ++ctx->upload_slow;
  }
  return VGICP_OK;
}

// A scan upload in three steps — stage (everything up to the copy), crew_post + crew_join (the copy threads), finish — so
// that the fused align can put its launch between the first two (vgicp_align).
struct UploadJob {
  bool staged = false;         // false: scan_upload_stage did the whole upload (n == 0 or the runtime's copy)
  double t0 = 0.0;
  CopyJob copy;
};

// The scan's bookkeeping; a staged upload's memory and its copy job (not posted yet).  A scan that is not staged is
// enqueued here whole (copies + pack_scan_kernel).
int scan_upload_stage(vgicp_ctx* ctx, size_t n, const double* points, const double* covs, UploadJob* up) {
  *up = UploadJob{};
  if (n > 0 && (!points || !covs)) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL scan pointer");
  if (n > 0xFFFFFFFFull) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "scan too large");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(begin_scan(ctx, n, 0.0, false));
  ctx->n = (uint32_t)n;
  if (n == 0) return VGICP_OK;
  up->t0 = now_seconds();
  double* aos_pts = ctx->d_scan_aos;
  double* aos_cov = ctx->d_scan_aos + 3 * ctx->scan_capacity;
  next_nonzero(ctx->scan_seq);
  ctx->scan_sym_known = true;
  const size_t bytes = n * kScanPlanes * sizeof(double);
  if (!upload_is_staged(ctx, n, points, covs)) {
    VG_HIP(ctx, hipMemcpyAsync(aos_pts, points, n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    VG_HIP(ctx, hipMemcpyAsync(aos_cov, covs, n * 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    VG_HIP(ctx, launch_pack_scan(ctx->stream, aos_pts, aos_cov, (uint32_t)n, ctx->d_scan, ctx->stride,
                                 ctx->d_ins_counters + 2, ctx->scan_seq));
    ctx->upload_bytes += bytes;
    ctx->upload_seconds += now_seconds() - up->t0;  // host side: the copy calls + the enqueue of the pack kernel
    return VGICP_OK;
  }
  const size_t pb = align256(n * 3 * sizeof(double) + 16), cb = align256(n * 9 * sizeof(double) + 16);
  VG_RC(ensure_upload_stage(ctx, pb + cb));
  if (!ctx->ev_upload) VG_HIP(ctx, ctx->ev_upload.create(false));
  // the kernel that read the staging memory last has long finished (every align ends in a synchronisation); make sure
  if (ctx->upload_in_flight && hipEventQuery(ctx->ev_upload) != hipSuccess) VG_HIP(ctx, hipEventSynchronize(ctx->ev_upload));
  ctx->upload_in_flight = false;
  up->staged = true;
  CopyJob& job = up->copy;
  job.flags = reinterpret_cast<uint32_t*>(ctx->h_upload.get());
  job.src_a = points, job.dst_a = ctx->h_upload + ctx->upload_flag_bytes, job.size_a = 3 * sizeof(double);
  job.src_b = covs, job.dst_b = job.dst_a + pb, job.size_b = 9 * sizeof(double), job.copy_b_form = stage_cov_unit;
  job.n = n, job.seq = ctx->scan_seq;
  job.bytes = bytes, job.wake_bytes = 2u << 20;
  return VGICP_OK;
}

// The end of a launch that read the staging memory AND is waited for by its caller (the fused align): the
// synchronisation itself proves that the staging memory is free again, so no marker is recorded behind the launch (one
// packet less between the kernel's end and the caller's return) and upload_in_flight — "a launch may still be reading
// the staging memory; ev_upload says when it has" — stays false, which is all that ensure_upload_stage and
// scan_upload_stage ask.  Only a synchronisation that fails leaves the marker behind after all.  (vgicp_scan_upload's
// enqueue and the two-launch vgicp_align do not end in a wait of their own: they keep the marker.)
int staged_launch_synchronise(vgicp_ctx* ctx) {
  ctx->upload_in_flight = false;
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) return VGICP_OK;
  if (hipEventRecord(ctx->ev_upload, ctx->stream) == hipSuccess) ctx->upload_in_flight = true;
  return fail_hip(ctx, e, "hipStreamSynchronize(ctx->stream)");
}

// pack_arena_kernel over the staging memory of the current scan (wait: behind the copy threads, with the pack's patience)
hipError_t launch_pack_staged(vgicp_ctx* ctx, bool wait) {
  const uint32_t spin_limit = ctx->dev.pack_spin_limit ? ctx->dev.pack_spin_limit : kPackSpinLimit;
  CopyCrew* crew = ctx->crew.get();
  return launch_pack_arena(ctx->stream, crew->apts, crew->acov, ctx->n, crew->flags, wait, ctx->scan_seq, wait ? spin_limit : 0,
                           ctx->d_scan_aos, ctx->d_scan_aos + 3 * ctx->scan_capacity, ctx->d_scan, ctx->stride,
                           ctx->d_ins_counters + 2);
}

// The whole upload, enqueued: the pack kernel (and whatever the caller enqueues next) runs in stream order.
int scan_upload_enqueue(vgicp_ctx* ctx, size_t n, const double* points, const double* covs) {
  UploadJob up;
  int rc = scan_upload_stage(ctx, n, points, covs, &up);
  if (rc != VGICP_OK || !up.staged) return rc;
  crew_post(ctx, &up.copy);
  // the launch first (it starts reading as soon as unit 0 is published), then this thread copies too
  const hipError_t e_launch = launch_pack_staged(ctx, true);
  bool slow = false;
  rc = crew_join(ctx, up.copy, &slow);
  if (e_launch != hipSuccess) return fail_hip(ctx, e_launch, "launch_pack_arena");
  if (rc != VGICP_OK) return rc;
  // the copy threads were held up for so long that a workgroup of the launch may have stopped waiting: everything is
  // staged now, pack it again behind the launch (no flags to wait for)
  if (slow) VG_HIP(ctx, launch_pack_staged(ctx, false));
  VG_HIP(ctx, hipEventRecord(ctx->ev_upload, ctx->stream));
  ctx->upload_in_flight = true;
  ctx->upload_bytes += n * kScanPlanes * sizeof(double);
  ctx->upload_seconds += now_seconds() - up.t0;  // host side: the staging copy + the enqueue of the pack kernel
  return VGICP_OK;
}
}  // namespace

int vgicp_scan_upload(vgicp_ctx* ctx, size_t n, const double* points, const double* covs) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::scan_upload(ctx, n, points, covs);
  VG_RC(settle(ctx));
  int rc = scan_upload_enqueue(ctx, n, points, covs);
  if (rc != VGICP_OK) return rc;
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->scan_ready = true;
  return VGICP_OK;
}

int vgicp_host_register(vgicp_ctx* ctx, const void* buffer, size_t bytes) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (!buffer || bytes == 0) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL / empty buffer");
  if (ctx->multi) {  // page-locked once, for every device (portable)
    VG_HIP(ctx, hipHostRegister(const_cast<void*>(buffer), bytes, hipHostRegisterPortable));
    return VGICP_OK;
  }
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_HIP(ctx, hipHostRegister(const_cast<void*>(buffer), bytes, hipHostRegisterDefault));
  return VGICP_OK;
}

int vgicp_host_unregister(vgicp_ctx* ctx, const void* buffer) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (!buffer) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL buffer");
  if (ctx->multi) {
    size_t unused = 0;
    const int rc_sync = vgicp_multi_api::map_size(ctx, &unused, nullptr);  // settles every sub-context: no copy in flight
    if (rc_sync != VGICP_OK) return rc_sync;
    VG_HIP(ctx, hipHostUnregister(const_cast<void*>(buffer)));
    return VGICP_OK;
  }
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));  // no copy out of the buffer may still be in flight
  VG_HIP(ctx, hipHostUnregister(const_cast<void*>(buffer)));
  return VGICP_OK;
}
}  // extern "C"
