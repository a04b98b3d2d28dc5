// vgicp_capi_multi_support.inl — part of vgicp_capi.hip.
// ---------------------------------------------------------------------------------------------------------------
// What the in-process multi-device context (vgicp_multi.hip) needs from this file besides the entry points above.
// ---------------------------------------------------------------------------------------------------------------
namespace vgicp_internal {

int settle_context(vgicp_ctx* ctx) { return settle(ctx); }

// Whether an align of n points / max_it rounds would have to (re)allocate on this context, and the allocation itself.
// hipFree waits for the whole DEVICE: sub-contexts that share a device must not meet one between their launches (a
// neighbour's persistent kernel is already running and waiting for this sub-context's), so the multi-device context
// grows every sub-context's buffers in a phase of its own before anybody launches.
bool align_needs_allocation(const vgicp_ctx* ctx, size_t n, int max_it) {
  // (the dense copy's storage is made when the table is: reserve_dense; an align only rebuilds its contents)
  return !ctx->d_scan || n > ctx->scan_capacity || max_it > ctx->log_capacity || ctx->log_capacity == 0;
}
int reserve_for_align(vgicp_ctx* ctx, size_t n, int max_it) {
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!ctx->d_scan || n > ctx->scan_capacity) {
    VG_RC(ensure_scan(ctx, n));
    ctx->scan_ready = false;   // whatever was resident went with the old buffers
    ctx->n = 0;
    forget_fetch(ctx);
  }
  return ensure_log(ctx, std::max(max_it, 1));
}

int wire_mailboxes(vgicp_ctx* const* subs, int n) {
  if (n < 1 || n > kMaxRanks) return fail(subs[0], VGICP_ERR_BAD_ARGUMENT, "at most 16 devices");
  // every device must be able to store into every other device's mailbox (xGMI / PCIe peer access)
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      if (subs[a]->device == subs[b]->device) continue;
      int can = 0;
      VG_HIP(subs[a], hipDeviceCanAccessPeer(&can, subs[a]->device, subs[b]->device));
      if (!can) return fail(subs[a], VGICP_ERR_HIP, "device " + std::to_string(subs[a]->device) + " cannot access device " +
                            std::to_string(subs[b]->device) + " as a peer");
      VG_HIP(subs[a], hipSetDevice(subs[a]->device));
      const hipError_t e = hipDeviceEnablePeerAccess(subs[b]->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail_hip(subs[a], e, "hipDeviceEnablePeerAccess");
      (void)hipGetLastError();
    }
  for (int r = 0; r < n; ++r) {
    vgicp_ctx* ctx = subs[r];
    VG_HIP(ctx, hipSetDevice(ctx->device));
    VG_RC(ensure_mailbox(ctx));
    // this rank's mailbox: the rows the ranks write are unset, the others +0.0 for good; verdict words 0
    std::vector<unsigned long long> img(kMailWords, 0ull);
    for (int buf = 0; buf < 3; ++buf)
      for (int q = 0; q < n; ++q)
        for (int sl = 0; sl <= kCountSlot; ++sl) img[((size_t)buf * kMaxRanks + q) * kSlots + sl] = kRowUnset;
    VG_HIP(ctx, hipMemcpy(ctx->d_mail, img.data(), kMailWords * 8, hipMemcpyHostToDevice));
  }
  for (int r = 0; r < n; ++r) {
    vgicp_ctx* ctx = subs[r];
    VG_HIP(ctx, hipSetDevice(ctx->device));
    for (int q = 0; q < kMaxRanks; ++q) ctx->peer_mail[q] = q < n ? subs[q]->d_mail : nullptr;
    VG_HIP(ctx, hipMemcpy(ctx->d_mail_table, ctx->peer_mail, kMaxRanks * sizeof(double*), hipMemcpyHostToDevice));
    ctx->peer_mail_is_ipc = false;
    ctx->peer_world = n;
    ctx->peer_rank = r;
    ctx->world_size = n;
    ctx->rank = r;
    ctx->mail_round0 = 0;
    ctx->mail_seq = 0;
    ctx->peer_enabled = true;
    ctx->peers_connected = true;
  }
  return VGICP_OK;
}

namespace {
// tree_sum<16> of vgicp_kernels.hip on the host: the order in which poll_and_sum<true> adds the ranks' rows
double tree_sum_host(const double* v, int count) {
  if (count == 1) return v[0];
  return tree_sum_host(v, count / 2) + tree_sum_host(v + count / 2, count - count / 2);
}
}  // namespace

// The group's form of align_on_loop: the same launches on every device, `prev` is the row the HOST summed over the ranks
// between the launches (one synchronisation per round); the lead device's events and log make the report.
int align_host_summed(vgicp_ctx* const* subs, int n, const double guess[16], const vgicp_params* params,
                      double out_pose[16], vgicp_stats* stats) {
  const double t0 = now_seconds();
  vgicp_ctx* lead = subs[0];
  VG_RC(check_params(lead, params));
  const int max_it = params->max_iteration;
  const bool profile = (params->flags & VGICP_FLAG_PROFILE) != 0;
  std::vector<uint32_t> grid((size_t)n);
  for (int r = 0; r < n; ++r) {
    vgicp_ctx* ctx = subs[r];
    VG_HIP(ctx, hipSetDevice(ctx->device));
    VG_RC(settle(ctx));
    VG_RC(align_ready(ctx, params));
    VG_RC(upload_initial_state(ctx, guess, params));
    grid[(size_t)r] = iterate_grid(ctx);
  }
  VG_HIP(lead, hipSetDevice(lead->device));
  int total_launches = 0;
  VG_RC(loop_launches(lead, params, &total_launches));
  VG_HIP(lead, hipEventRecord(lead->ev_begin, lead->stream));
  int launched = 0;
  for (int j = 0; j < total_launches; ++j) {
    const bool closing = j == max_it;
    for (int r = 0; r < n; ++r) {
      vgicp_ctx* ctx = subs[r];
      VG_HIP(ctx, hipSetDevice(ctx->device));
      const IterArgs a = launch_args(ctx, base_args(ctx), j, grid[(size_t)r], /*summed=*/true);
      if (profile && r == 0) VG_HIP(ctx, hipEventRecord(ctx->ev_prof[2 * j], ctx->stream));
      if (closing) VG_HIP(ctx, launch_close(ctx->stream, a, ctx->iter_block));
      else {
        VG_HIP(ctx, launch_iterate(ctx->stream, a, grid[(size_t)r], ctx->iter_block));
        VG_HIP(ctx, launch_fold_rows(ctx->stream, a.rows, grid[(size_t)r], a.state_out, ctx->d_sums));
        // the rank's row goes to pinned memory (the header row of the pinned log: unused outside a persistent launch)
        VG_HIP(ctx, hipMemcpyAsync(ctx->h_log, ctx->d_sums, kSlots * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      }
      if (profile && r == 0) VG_HIP(ctx, hipEventRecord(ctx->ev_prof[2 * j + 1], ctx->stream));
      VG_HIP(ctx, hipMemcpyAsync(&ctx->h_state[1], a.state_out, sizeof(AlignState), hipMemcpyDeviceToHost, ctx->stream));
    }
    ++launched;
    for (int r = 0; r < n; ++r) {
      VG_HIP(subs[r], hipSetDevice(subs[r]->device));
      VG_HIP(subs[r], hipStreamSynchronize(subs[r]->stream));
    }
    if (closing || lead->h_state[1].done) break;
    // the ranks' rows, added in the order the mailbox path adds them (identical bits on every device)
    double total[kSlots];
    for (int sl = 0; sl < kSlots; ++sl) {
      double x[kMaxRanks];
      for (int q = 0; q < kMaxRanks; ++q) x[q] = (q < n && sl <= kCountSlot) ? subs[q]->h_log[sl] : 0.0;
      total[sl] = tree_sum_host(x, kMaxRanks);
    }
    for (int r = 0; r < n; ++r) {
      vgicp_ctx* ctx = subs[r];
      VG_HIP(ctx, hipSetDevice(ctx->device));
      std::memcpy(ctx->h_log, total, sizeof total);
      VG_HIP(ctx, hipMemcpyAsync(ctx->d_sums, ctx->h_log, kSlots * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
  }
  VG_HIP(lead, hipSetDevice(lead->device));
  return report_loop(lead, params, launched, n, t0, out_pose, stats);
}

int adopt_device_scan(vgicp_ctx* ctx, int src_device, const double* d_points, const double* d_covs, size_t n,
                      double prep_voxel, hipEvent_t ready) {
  if (n > 0xFFFFFFFFull) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "scan too large");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  VG_RC(begin_scan(ctx, n, prep_voxel, false));   // the source's down-sampling still describes the points
  ctx->n = (uint32_t)n;
  if (ready) VG_HIP(ctx, hipStreamWaitEvent(ctx->stream, ready, 0));
  if (n > 0) {
    double* aos_pts = ctx->d_scan_aos;
    double* aos_cov = ctx->d_scan_aos + 3 * ctx->scan_capacity;
    if (src_device != ctx->device) {
      VG_HIP(ctx, hipMemcpyPeerAsync(aos_pts, ctx->device, d_points, src_device, n * 3 * sizeof(double), ctx->stream));
      VG_HIP(ctx, hipMemcpyPeerAsync(aos_cov, ctx->device, d_covs, src_device, n * 9 * sizeof(double), ctx->stream));
      g_copy_ops += 2;
    } else {
      VG_HIP(ctx, hipMemcpyAsync(aos_pts, d_points, n * 3 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      VG_HIP(ctx, hipMemcpyAsync(aos_cov, d_covs, n * 9 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    next_nonzero(ctx->scan_seq);
    ctx->scan_sym_known = true;
    VG_HIP(ctx, launch_pack_scan(ctx->stream, aos_pts, aos_cov, (uint32_t)n, ctx->d_scan, ctx->stride,
                                 ctx->d_ins_counters + 2, ctx->scan_seq));
  }
  ctx->scan_ready = true;
  return VGICP_OK;
}

int map_insert_device(vgicp_ctx* ctx, const double* d_points, const double* d_covs, size_t n, const double transform[16],
                      size_t max_points_per_voxel, bool short_lists, bool deferred, size_t* new_voxels) {
  if (new_voxels) *new_voxels = 0;
  const InsertVerdict v = insert_verdict(ctx, InsertEntry::Device, transform != nullptr, max_points_per_voxel, n);
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle_if_pending(ctx));
  if (v.nothing_to_do) return VGICP_OK;
  return insert_points(ctx, d_points, d_covs, n, transform, max_points_per_voxel, nullptr, short_lists, deferred, new_voxels);
}

}  // namespace vgicp_internal
