// vgicp_capi_registration.inl — part of vgicp_capi.hip.
// vgicp_align / vgicp_align_resident and the single-step hooks (accumulate, solve_step, match, voxel_index).
namespace {
// ---- the fused align: vgicp_align of a staged scan in ONE launch ----------------------------------------------------
// The persistent launch is enqueued while the copy threads stage the scan; each workgroup waits for the staged unit(s)
// that hold its 448 points and reads them over PCIe itself (fused_round0_load), so neither pack_arena_kernel, nor the
// kernel boundary, nor the re-read of the planes stand between the last unit and round 0; the resident copy leaves the
// launch behind round 0's row publication (fused_leave_resident).  The helpers are posted as soon as the copy job is
// complete, before the launch is set up, and the launch is followed by the synchronisation alone, without a marker
// (staged_launch_synchronise).  Where it is taken: plan_align (AlignPath::Fused); everything else keeps the pack launch
// in front.
int align_fused(vgicp_ctx* ctx, size_t n, const double* points, const double* covs, const double* guess,
                const vgicp_params* params, double* out_pose, vgicp_stats* stats) {
  const double t0 = now_seconds();
  VG_RC(check_params(ctx, params));
  VG_RC(ensure_log(ctx, params->max_iteration));
  UploadJob up;
  VG_RC(scan_upload_stage(ctx, n, points, covs, &up));
  // the copy job is complete: the helpers start on their first units while this thread sets the launch up (the link is
  // idle until the first unit is staged)
  crew_post(ctx, &up.copy);
  PersistArgs a;
  const int rc_args = persistent_args(ctx, guess, params, &a);
  if (rc_args != VGICP_OK) {   // no launch: the copy threads still have to let go of the caller's buffers
    bool held_up = false;
    const int rc_join = crew_join(ctx, up.copy, &held_up);
    return rc_join != VGICP_OK ? rc_join : rc_args;
  }
  FusedUpload f;
  std::memset(&f, 0, sizeof f);
  f.apts = up.copy.dst_a;
  f.acov = up.copy.dst_b;
  f.flags = up.copy.flags;
  f.unit = pack_arena_unit();
  f.seq = ctx->scan_seq;
  f.spin_limit = ctx->dev.pack_spin_limit ? ctx->dev.pack_spin_limit : kPackSpinLimit;
  f.soa = ctx->d_scan;
  f.aos_pts = ctx->d_scan_aos;
  f.aos_cov = ctx->d_scan_aos + 3 * ctx->scan_capacity;
  f.asym = ctx->d_ins_counters + 2;
  f.unit_clock = ctx->d_unit_clock;
  const bool trace = trace_align();   // where the host time goes
  const double ta0 = trace ? now_seconds() : 0.0;
  const hipError_t e_launch = launch_persistent_fused(ctx->stream, a, f, ctx->persist_grid);
  const double ta1 = trace ? now_seconds() : 0.0;
  bool slow = false;
  const int rc = crew_join(ctx, up.copy, &slow);
  if (rc != VGICP_OK) {
    // a copy thread never delivered: the launch has given up waiting for its unit by now (crew_gave_up synchronised)
    (void)reset_persistent_exchange(ctx);
    return rc;
  }
  if (e_launch != hipSuccess) return fail_hip(ctx, e_launch, "launch_persistent_fused");
  const double ta2 = trace ? now_seconds() : 0.0;
  ctx->upload_bytes += n * kScanPlanes * sizeof(double);
  ctx->upload_seconds += now_seconds() - up.t0;  // host side: the staging copy + the enqueue of the launch
  ctx->scan_ready = true;
  VG_RC(staged_launch_synchronise(ctx));   // no marker behind the launch: this wait is what frees the staging memory
  const double ta3 = trace ? now_seconds() : 0.0;
  if (trace && ta3 - ta0 > 2e-3)
    std::fprintf(stderr, "[vgicp trace] fused align: enqueue %.3f ms, copy %.3f ms, hipStreamSynchronize %.3f ms\n",
                 (ta1 - ta0) * 1e3, (ta2 - ta1) * 1e3, (ta3 - ta2) * 1e3);
  ++ctx->persistent_launches;
  AlignState* hf = &ctx->h_state[0];
  std::memcpy(hf, reinterpret_cast<const AlignState*>(ctx->h_log.get()), sizeof(AlignState));
  VG_RC(settle_after_launch(ctx, *hf, a.seq, /*multi=*/false));
  if (!launch_committed(*hf, a.seq, hf->abort_seq)) {
    // A wait inside the launch ran out.  The copy threads have delivered everything by now: pack the scan behind the
    // launch (no flags to wait for), put the exchange back into its initial state and run the align again.  Copy threads
    // that were held up (counted once, as slow) explain it: the single launch is simply repeated.  Otherwise the device
    // did not have every workgroup resident: a persistent fallback, this align goes to the loop.
    VG_HIP(ctx, launch_pack_staged(ctx, false));
    VG_RC(reset_persistent_exchange(ctx));
    if (slow) return run_align(ctx, guess, params, out_pose, stats);
    count_fallback(ctx, "persistent align launch gave up waiting for a workgroup", "");
    return align_on_loop(ctx, guess, params, out_pose, stats, now_seconds());
  }
  advance_exchange(ctx, *hf, /*multi=*/false);
  // the registration's device time, the upload excluded: from the moment the last workgroup found its units to the
  // end of the launch, on the device's constant clock
  const double device_seconds = ctx->wall_clock_hz > 0.0 ? (double)hf->unit_to_end_ticks / ctx->wall_clock_hz : 0.0;
  return report_align(ctx, *hf, ctx->h_log_rows(), 1, 1, device_seconds, t0, out_pose, stats);
}
}  // namespace

extern "C" {

int vgicp_align_resident(vgicp_ctx* ctx, const double guess[16], const vgicp_params* params,
                         double out_pose[16], vgicp_stats* stats) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (!guess || !out_pose) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL pose pointer");
  if (ctx->multi) return vgicp_multi_api::align_resident(ctx, guess, params, out_pose, stats);
  VG_HIP(ctx, hipSetDevice(ctx->device));
  return run_align(ctx, guess, params, out_pose, stats);
}

int vgicp_align(vgicp_ctx* ctx, size_t n, const double* points, const double* covs,
                const double guess[16], const vgicp_params* params, double out_pose[16],
                vgicp_stats* stats) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) {
    if (!guess || !out_pose) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL pose pointer");
    return vgicp_multi_api::align(ctx, n, points, covs, guess, params, out_pose, stats);
  }
  VG_RC(settle(ctx));
  const double t0 = now_seconds();
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  AlignFacts facts = align_facts(ctx, params, AlignCall::Upload, n);
  facts.buffers = params && points && covs && guess && out_pose;
  facts.upload_staged = true;   // asked last, and only when everything else says Fused: it looks the caller's pointers up
  if (plan_align(facts).path == AlignPath::Fused && upload_is_staged(ctx, n, points, covs)) {
    VG_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = align_fused(ctx, n, points, covs, guess, params, out_pose, stats);   // one launch
    if (stats) stats->seconds = now_seconds() - t0;
    return rc;
  }
  // the upload is only enqueued: the pack kernel and the align's first launch follow it in stream order
  int rc = scan_upload_enqueue(ctx, n, points, covs);
  if (rc != VGICP_OK) return rc;
  ctx->scan_ready = true;
  rc = vgicp_align_resident(ctx, guess, params, out_pose, stats);
  if (stats) stats->seconds = now_seconds() - t0;
  return rc;
}

int vgicp_accumulate(vgicp_ctx* ctx, size_t n, const double* points, const double* covs,
                     const double pose[16], double JTJ[36], double JTr[6], uint64_t* count) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) {  // a hook that works on one device ("local rank only"): the whole scan on sub-context 0
    vgicp_multi_api::scan_replaced(ctx);
    return forward_to_first(ctx, [&](vgicp_ctx* first) { return vgicp_accumulate(first, n, points, covs, pose, JTJ, JTr, count); });
  }
  if (!pose || !JTJ || !JTr) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL output pointer");
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  int rc = vgicp_scan_upload(ctx, n, points, covs);
  if (rc != VGICP_OK) return rc;
  rc = ensure_log(ctx, 1);
  if (rc != VGICP_OK) return rc;
  AlignState* h0 = &ctx->h_state[0];
  std::memset(h0, 0, sizeof(AlignState));
  pose_to_state(pose, h0->pose);
  h0->cosine_threshold = 2.0;
  h0->max_iteration = 1;
  VG_HIP(ctx, hipMemcpyAsync(ctx->d_state, h0, sizeof(AlignState), hipMemcpyHostToDevice, ctx->stream));
  // local rank only (never the communicator): one body launch, then the closing prologue
  const IterArgs base = base_args(ctx);
  const uint32_t grid = iterate_grid(ctx);
  rc = enqueue_launch(ctx, base, 0, grid, false, false);
  if (rc != VGICP_OK) return rc;
  rc = enqueue_launch(ctx, base, 1, grid, true, false);
  if (rc != VGICP_OK) return rc;
  VG_HIP(ctx, hipMemcpyAsync(ctx->h_log_rows(), ctx->d_log_rows(), kSlots * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const double* row = ctx->h_log_rows();
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c <= r; ++c) {
      JTJ[r + 6 * c] = row[tri6(r, c)];
      JTJ[c + 6 * r] = row[tri6(r, c)];
    }
  for (int k = 0; k < 6; ++k) JTr[k] = row[21 + k];
  if (count) *count = (uint64_t)row[kCountSlot];
  return VGICP_OK;
}

int vgicp_solve_step(vgicp_ctx* ctx, const double JTJ[36], const double JTr[6], double cosine_threshold,
                     double translation_sq_threshold, uint32_t flags, double se3[6], double step[16],
                     int32_t* used_pivoted, int32_t* converged) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi)
    return forward_to_first(ctx, [&](vgicp_ctx* first) {
      return vgicp_solve_step(first, JTJ, JTr, cosine_threshold, translation_sq_threshold, flags, se3, step, used_pivoted, converged);
    });
  if (!JTJ || !JTr || !se3 || !step) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage(ctx, 64 * sizeof(double));
  if (rc != VGICP_OK) return rc;
  double packed[32] = {0.0};
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c <= r; ++c) packed[tri6(r, c)] = JTJ[r + 6 * c];  // the lower triangle, as Eigen's LDLT reads it
  for (int k = 0; k < 6; ++k) packed[21 + k] = JTr[k];
  double* d_in = static_cast<double*>(ctx->d_stage.get());
  double* d_out = d_in + 32;
  double out[20];
  VG_HIP(ctx, hipMemcpyAsync(d_in, packed, sizeof packed, hipMemcpyHostToDevice, ctx->stream));
  VG_HIP(ctx, launch_solve_step(ctx->stream, d_in, cosine_threshold, translation_sq_threshold,
                                (flags & VGICP_SOLVE_FORCE_PIVOTED) ? 1 : 0, d_out));
  VG_HIP(ctx, hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 6; ++k) se3[k] = out[k];
  Pose T;
  for (int k = 0; k < 9; ++k) T.R[k] = out[6 + k];
  for (int k = 0; k < 3; ++k) T.t[k] = out[15 + k];
  pose_to_mat4(T, step);
  if (used_pivoted) *used_pivoted = out[18] != 0.0;
  if (converged) *converged = out[19] != 0.0;
  return VGICP_OK;
}

int vgicp_match(vgicp_ctx* ctx, size_t n, const double* points, const double* covs,
                double* src_points, double* src_covs, double* map_points, double* map_covs,
                uint64_t* src_index, size_t* matched) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi)   // the map is replicated: any replica answers
    return forward_to_first(ctx, [&](vgicp_ctx* first) {
      return vgicp_match(first, n, points, covs, src_points, src_covs, map_points, map_covs, src_index, matched);
    });
  if (!matched) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "matched is NULL");
  *matched = 0;
  VG_RC(settle(ctx));
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (n == 0) return VGICP_OK;
  if (!points || !covs || !src_points || !src_covs || !map_points || !map_covs)
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL array pointer");
  if (n > 0xFFFFFFFFull) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "scan too large");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t nb = match_blocks((uint32_t)n);
  // staging layout: in_pts | in_cov | out src_pts | src_cov | map_pts | map_cov | index | counts | total
  const size_t pb = n * 3 * sizeof(double), cb = n * 9 * sizeof(double);
  StageLayout lay;
  const size_t o_in_pts = lay.take(pb), o_in_cov = lay.take(cb), o_sp = lay.take(pb), o_sc = lay.take(cb), o_mp = lay.take(pb);
  const size_t o_mc = lay.take(cb), o_ix = lay.take(n * sizeof(uint64_t)), o_counts = lay.take((size_t)nb * sizeof(uint32_t));
  const size_t o_total = lay.take(sizeof(uint32_t));
  VG_RC(ensure_stage(ctx, lay.total));
  double *in_pts = stage_at<double>(ctx, o_in_pts), *in_cov = stage_at<double>(ctx, o_in_cov);
  double *o_src_p = stage_at<double>(ctx, o_sp), *o_src_c = stage_at<double>(ctx, o_sc);
  double *o_map_p = stage_at<double>(ctx, o_mp), *o_map_c = stage_at<double>(ctx, o_mc);
  uint64_t* o_index = stage_at<uint64_t>(ctx, o_ix);
  uint32_t *counts = stage_at<uint32_t>(ctx, o_counts), *d_total = stage_at<uint32_t>(ctx, o_total);
  arena_reset(ctx);
  VG_RC(user_h2d(ctx, in_pts, points, pb));
  VG_RC(user_h2d(ctx, in_cov, covs, cb));
  VG_HIP(ctx, launch_match(ctx->stream, in_pts, in_cov, (uint32_t)n, ctx->table,
                           (uint32_t)(ctx->slots - 1), ctx->voxel_size, counts, d_total, o_src_p, o_src_c,
                           o_map_p, o_map_c, o_index));
  VG_HIP(ctx, hipMemcpyAsync(ctx->h_counters, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t m = ctx->h_counters[0];
  if (m > 0) {
    arena_reset(ctx);   // the inputs have been consumed (synchronised above)
    VG_RC(user_d2h(ctx, src_points, o_src_p, m * 3 * sizeof(double)));
    VG_RC(user_d2h(ctx, src_covs, o_src_c, m * 9 * sizeof(double)));
    VG_RC(user_d2h(ctx, map_points, o_map_p, m * 3 * sizeof(double)));
    VG_RC(user_d2h(ctx, map_covs, o_map_c, m * 9 * sizeof(double)));
    if (src_index) VG_RC(user_d2h(ctx, src_index, o_index, m * sizeof(uint64_t)));
    VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    user_copies_finish(ctx);
  }
  *matched = m;
  return VGICP_OK;
}

int vgicp_voxel_index(vgicp_ctx* ctx, size_t n, const double* points, int32_t* keys) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return forward_to_first(ctx, [&](vgicp_ctx* first) { return vgicp_voxel_index(first, n, points, keys); });
  VG_RC(settle(ctx));
  if (n == 0) return VGICP_OK;
  if (!points || !keys) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL array pointer");
  if (!(ctx->voxel_size > 0.0)) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel size: call vgicp_map_reset first");
  if (n > 0xFFFFFFFFull) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "scan too large");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  const size_t pb = n * 3 * sizeof(double), kb = n * 3 * sizeof(int32_t);
  int rc = ensure_stage(ctx, pb + kb);
  if (rc != VGICP_OK) return rc;
  char* b = static_cast<char*>(ctx->d_stage.get());
  arena_reset(ctx);
  VG_RC(user_h2d(ctx, b, points, pb));
  VG_HIP(ctx, launch_voxel_index(ctx->stream, reinterpret_cast<const double*>(b), (uint32_t)n,
                                 ctx->voxel_size, reinterpret_cast<int32_t*>(b + pb)));
  VG_RC(user_d2h(ctx, keys, b + pb, kb));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  user_copies_finish(ctx);
  return VGICP_OK;
}
}  // extern "C"
