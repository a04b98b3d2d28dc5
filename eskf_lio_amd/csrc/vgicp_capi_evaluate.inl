// vgicp_capi_evaluate.inl — part of vgicp_capi.hip.
// vgicp_evaluate_resident (include/vgicp_hip_evaluate.h): argument checks, settling, the launch pairs with their one
// synchronisation, the report.  Reads the context; writes only the evaluation's own storage (d_eval_rows, h_eval).
extern "C" {

int vgicp_evaluate_resident(vgicp_ctx* ctx, size_t k, const double* poses, vgicp_evaluation* out, vgicp_eval_stats* stats) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (k < 1 || k > (size_t)VGICP_EVAL_MAX) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "k must be 1 .. VGICP_EVAL_MAX");
  if (!poses || !out) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  for (size_t i = 0; i < 16 * k; ++i)
    if (!std::isfinite(poses[i]))
      return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "pose " + std::to_string(i / 16) + " has an entry that is not finite");
  if (ctx->multi || ctx->owner || ctx->comm || ctx->peers_connected)
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "vgicp_evaluate_resident is not available on multi-device contexts, communicators "
                "and peer-connected contexts: the resident scan of a device is a shard there");
  const double t0 = now_seconds();
  VG_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (!ctx->scan_ready) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  // the launch geometry is made from the kept count: a pending scan (and a pending insertion with it) is settled first
  VG_RC(settle(ctx));
  if (!ctx->scan_ready) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident");

  const uint32_t rows = iterate_grid(ctx->n, 512);   // workgroups per pose: the grid of the loop's 512-thread launch
  const size_t per_launch = std::min<size_t>(VGICP_EVAL_MAX, (size_t)kEvalRowBudget / rows);
  double* h_poses = ctx->h_eval + (size_t)VGICP_EVAL_MAX * kSlots;
  for (size_t h = 0; h < k; ++h) pose_to_state(poses + 16 * h, h_poses + 12 * h);
  EvalArgs a;
  std::memset(&a, 0, sizeof a);
  static_cast<ResidentView&>(a) = resident_view(ctx);
  a.rows = ctx->d_eval_rows;
  a.scan_seq = ctx->scan_seq;
  a.asym_dev = symmetry_word(ctx);
  int launches = 0;
  VG_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
  for (size_t h0 = 0; h0 < k; h0 += per_launch) {
    const uint32_t m = (uint32_t)std::min<size_t>(per_launch, k - h0);
    a.poses = ctx->h_eval.dev() + (size_t)VGICP_EVAL_MAX * kSlots + 12 * h0;
    // stream order: this pair's rows are written after the previous pair's fold has read its own
    VG_HIP(ctx, launch_evaluate(ctx->stream, a, rows, m));
    VG_HIP(ctx, launch_evaluate_fold(ctx->stream, ctx->d_eval_rows, rows, m, ctx->h_eval.dev() + h0 * kSlots));
    launches += 2;
  }
  VG_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t h = 0; h < k; ++h) {
    const double* row = ctx->h_eval + h * kSlots;
    out[h].points = ctx->n;
    out[h].correspondences = (uint64_t)row[kCountSlot];
    out[h].cost = row[kCostSlot];
    out[h].sq_error = row[kSqErrorSlot];
    for (int s = 0; s < kNormalEq; ++s) out[h].normal_eq[s] = row[s];
  }
  if (stats) {
    float ms = 0.f;
    VG_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
    stats->launches = launches;
    stats->poses_per_launch = (int32_t)per_launch;
    stats->seconds = now_seconds() - t0;
    stats->device_seconds = ms * 1e-3;
  }
  return VGICP_OK;
}
}  // extern "C"
