// vgicp_capi_batch.inl — part of vgicp_capi.hip.
// vgicp_align_resident_batch / vgicp_align_batch_width (include/vgicp_hip_batch.h): argument checks, settling, the team
// plan, the launches with their one synchronisation, the acceptance rule and the sequential paths through run_align.
namespace {
// How many hypotheses one team launch takes for the resident (settled) scan; 1 = a batch runs its aligns one by one.
// T = ceil(n / 448) workgroups per team, as many teams as fit the grid vgicp_create verified to be resident.
uint32_t batch_width(const vgicp_ctx* ctx, uint32_t* team_wgs) {
  *team_wgs = 0;
  const bool one_device = ctx->world_size == 1 && ctx->owner == nullptr && ctx->comm == nullptr && !ctx->peers_connected;
  if (!one_device || !ctx->persistent_enabled || ctx->d_stamps != nullptr || ctx->n == 0 ||
      (uint64_t)ctx->n > (uint64_t)ctx->persist_grid * 448u)
    return 1;
  const uint32_t T = (ctx->n + 447u) / 448u;
  const uint32_t width = std::min<uint32_t>((uint32_t)kTeamsMax, ctx->persist_grid / T);
  if (width < 2) return 1;
  *team_wgs = T;
  return width;
}

AlignState* batch_state(const vgicp_ctx* ctx, size_t h) {
  return reinterpret_cast<AlignState*>(ctx->h_batch + h * (size_t)kBatchSlotRows * kSlots);
}

void batch_report(size_t h, int max_it, const AlignState* st, const double* log, vgicp_batch_stats* stats) {
  if (!stats) return;
  if (stats->iterations) stats->iterations[h] = st->iteration;
  if (stats->converged) stats->converged[h] = st->converged;
  for (int it = 0; it < st->iteration; ++it) {
    const double* row = log + (size_t)it * kSlots;
    if (stats->corr_count) stats->corr_count[h * (size_t)max_it + it] = (uint64_t)row[kCountSlot];
    if (stats->normal_eq)
      std::memcpy(stats->normal_eq + (h * (size_t)max_it + it) * kNormalEq, row, kNormalEq * sizeof(double));
  }
}

// The k hypotheses as teams of persistent launches: ceil(k / width) launches back to back, ONE synchronisation.
// *ran = false: a workgroup gave up waiting (counted, cool-down set); the caller runs the batch on the loop.
int run_batch_teams(vgicp_ctx* ctx, size_t k, const double* guesses, const vgicp_params* params, uint32_t width,
                    uint32_t team_wgs, double* out_poses, vgicp_batch_stats* stats, int* first_bad, bool* ran) {
  static_assert(sizeof(AlignState) <= kSlots * sizeof(double), "the state must fit the header row of a hypothesis' block");
  *ran = false;
  const int max_it = params->max_iteration;
  const size_t slot_words = (size_t)kBatchSlotRows * kSlots;
  uint32_t* abort_host = reinterpret_cast<uint32_t*>(ctx->h_batch + (size_t)VGICP_BATCH_MAX * slot_words);
  PersistArgs a;
  std::memset(&a, 0, sizeof a);
  a.scan = ctx->d_scan;
  a.stride = ctx->stride;
  a.n = ctx->n;   // settled: the kept count
  a.mask = (uint32_t)(ctx->slots - 1);
  a.table = ctx->table;
  a.voxel_size = ctx->voxel_size;
  a.rows = ctx->d_batch_exchange;
  a.parts = ctx->d_batch_exchange + team_rows_words();
  a.spin_limit = ctx->persist_spin_limit;
  a.seq = ++ctx->persist_seq == 0 ? ++ctx->persist_seq : ctx->persist_seq;  // never 0; one number for the whole call
  a.cosine_threshold = params->cosine_threshold;
  a.translation_sq_threshold = params->translation_sq_threshold;
  a.max_iteration = max_it;
  a.round0 = 0;   // every launch starts from unset words
  a.world = 1;
  a.prefetch_margin = ctx->prefetch_margin;   // one point per thread, no memo, no stash: as the single launch has it
  TeamArgs t;
  std::memset(&t, 0, sizeof t);
  t.team_wgs = team_wgs;
  t.folder_rows = (team_wgs + kFolders - 1) / kFolders;
  t.slot_words = (uint32_t)slot_words;
  t.abort_word = reinterpret_cast<uint32_t*>(ctx->h_batch_dev + (size_t)VGICP_BATCH_MAX * slot_words);
  *abort_host = 0;
  for (size_t h = 0; h < k; ++h) {
    AlignState* st = batch_state(ctx, h);
    st->seq = 0;
    st->outcome = kOutcomeNone;
  }
  const size_t exchange_bytes = (team_rows_words() + team_parts_words()) * 8;
  int launches = 0;
  VG_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
  for (size_t h0 = 0; h0 < k; h0 += width, ++launches) {
    t.teams = (uint32_t)std::min<size_t>(width, k - h0);
    for (uint32_t h = 0; h < t.teams; ++h) pose_to_state(guesses + 16 * (h0 + h), t.pose0[h]);
    a.state = reinterpret_cast<AlignState*>(ctx->h_batch_dev + h0 * slot_words);
    a.log = ctx->h_batch_dev + h0 * slot_words + kSlots;
    // T, and with it the owner of every exchange word, changes with the scan, and teams end in different rounds: every
    // launch starts from words that are unset throughout (0xFF bytes = kRowUnset)
    VG_HIP(ctx, hipMemsetAsync(ctx->d_batch_exchange, 0xFF, exchange_bytes, ctx->stream));
    VG_HIP(ctx, launch_persistent_teams(ctx->stream, a, t, ctx->persist_grid));
  }
  VG_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  VG_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
  ctx->persistent_launches += (uint64_t)launches;
  // accepted only if every team's echo is there and nobody gave up (run_align_persistent's rule, k-wide)
  bool committed = *abort_host != a.seq;
  for (size_t h = 0; h < k && committed; ++h) {
    const AlignState* st = batch_state(ctx, h);
    committed = st->seq == a.seq && st->outcome == kOutcomeCommitted;
  }
  if (!committed) {
    ++ctx->persistent_fallbacks;
    ctx->persistent_cooldown = kPersistentCooldownAligns;
    if (ctx->persistent_fallbacks == 1 || ctx->dev.verbose)
      std::fprintf(stderr, "[vgicp] batched align launch gave up waiting for a workgroup (fallback #%llu): using one launch "
                   "per iteration for this batch and the next %d aligns\n", (unsigned long long)ctx->persistent_fallbacks,
                   kPersistentCooldownAligns);
    return VGICP_OK;
  }
  *ran = true;
  for (size_t h = 0; h < k; ++h) {
    const AlignState* st = batch_state(ctx, h);
    double* pose = out_poses + 16 * h;
    state_to_pose(st->pose, pose);
    batch_report(h, max_it, st, ctx->h_batch + h * slot_words + kSlots, stats);
    int status = VGICP_OK;
    if (!finite16(pose)) status = fail(ctx, VGICP_ERR_DEGENERATE, "solved pose is not finite (singular normal equations)");
    if (stats && stats->status) stats->status[h] = status;
    if (status != VGICP_OK && *first_bad == VGICP_OK) *first_bad = status;
  }
  if (stats) {
    stats->hypotheses_per_launch = (int32_t)std::min<size_t>(width, k);
    stats->launches = launches;
    stats->device_seconds = ms * 1e-3;
  }
  return VGICP_OK;
}
}  // namespace

// The k aligns one after another through the single call's own paths (also the multi-device forward); loop_only: on the
// launch-per-round loop without touching the cool-down.  Any status but VGICP_OK / VGICP_ERR_DEGENERATE ends the batch.
int vgicp_internal::align_batch_sequential(vgicp_ctx* ctx, size_t k, const double* guesses, const vgicp_params* params,
                                           double* out_poses, vgicp_batch_stats* stats, bool loop_only, int* first_bad) {
  const size_t max_it = (size_t)std::max(params->max_iteration, 0);
  int launches = 0;
  double device_seconds = 0.0;
  for (size_t h = 0; h < k; ++h) {
    vgicp_stats st;
    std::memset(&st, 0, sizeof st);
    if (stats && stats->corr_count) st.corr_count = stats->corr_count + h * max_it;
    if (stats && stats->normal_eq) st.normal_eq = stats->normal_eq + h * max_it * kNormalEq;
    const int rc = loop_only ? run_align(ctx, guesses + 16 * h, params, out_poses + 16 * h, &st, /*loop_only=*/true)
                             : vgicp_align_resident(ctx, guesses + 16 * h, params, out_poses + 16 * h, &st);
    if (rc != VGICP_OK && rc != VGICP_ERR_DEGENERATE) return rc;
    if (stats && stats->status) stats->status[h] = rc;
    if (stats && stats->iterations) stats->iterations[h] = st.iterations;
    if (stats && stats->converged) stats->converged[h] = st.converged;
    if (rc != VGICP_OK && *first_bad == VGICP_OK) *first_bad = rc;
    launches += st.launches;
    device_seconds += st.device_seconds;
  }
  if (stats) {
    stats->hypotheses_per_launch = 1;
    stats->launches = launches;
    stats->device_seconds = device_seconds;
  }
  return VGICP_OK;
}

extern "C" {

int vgicp_align_resident_batch(vgicp_ctx* ctx, size_t k, const double* guesses, const vgicp_params* params,
                               double* out_poses, vgicp_batch_stats* stats) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (k < 1 || k > (size_t)VGICP_BATCH_MAX) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "k must be 1 .. VGICP_BATCH_MAX");
  if (!guesses || !out_poses) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL pose pointer");
  { const int rc_params = check_params(ctx, params); if (rc_params != VGICP_OK) return rc_params; }
  const double t0 = now_seconds();
  int first_bad = VGICP_OK;
  int rc;
  if (ctx->multi) {
    rc = vgicp_multi_api::align_resident_batch(ctx, k, guesses, params, out_poses, stats, &first_bad);
    if (rc != VGICP_OK) return rc;
    if (stats) stats->seconds = now_seconds() - t0;
    return (stats && stats->status) ? VGICP_OK : first_bad;
  }
  VG_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (!ctx->scan_ready) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  // the team layout is made from the kept count: a pending scan (and a pending insertion with it) is settled first
  rc = settle(ctx);
  if (rc != VGICP_OK) return rc;
  if (!ctx->scan_ready) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident");
  const int max_it = params->max_iteration;
  uint32_t team_wgs = 0;
  const uint32_t width = batch_width(ctx, &team_wgs);
  const bool wide = k >= 2 && width >= 2 && max_it > 0 && max_it < kBatchSlotRows &&
                    (params->flags & (VGICP_FLAG_PROFILE | VGICP_FLAG_NO_PERSISTENT)) == 0;
  if (!wide) {
    rc = vgicp_internal::align_batch_sequential(ctx, k, guesses, params, out_poses, stats, /*loop_only=*/false, &first_bad);
  } else if (ctx->persistent_cooldown > 0) {
    // inside the cool-down no launch is attempted and nothing is counted: k aligns on the loop, k aligns of cool-down
    ctx->persistent_cooldown = std::max(0, ctx->persistent_cooldown - (int)k);
    rc = vgicp_internal::align_batch_sequential(ctx, k, guesses, params, out_poses, stats, /*loop_only=*/true, &first_bad);
  } else {
    bool ran = false;
    rc = run_batch_teams(ctx, k, guesses, params, width, team_wgs, out_poses, stats, &first_bad, &ran);
    if (rc == VGICP_OK && !ran)
      rc = vgicp_internal::align_batch_sequential(ctx, k, guesses, params, out_poses, stats, /*loop_only=*/true, &first_bad);
  }
  if (rc != VGICP_OK) return rc;
  if (stats) stats->seconds = now_seconds() - t0;
  return (stats && stats->status) ? VGICP_OK : first_bad;
}

int vgicp_align_batch_width(vgicp_ctx* ctx, size_t* hypotheses_per_launch) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (!hypotheses_per_launch) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "hypotheses_per_launch is NULL");
  *hypotheses_per_launch = 1;
  if (ctx->multi) return vgicp_multi_api::align_batch_width(ctx, hypotheses_per_launch);
  { const int rc_settle = settle(ctx); if (rc_settle != VGICP_OK) return rc_settle; }
  if (!ctx->scan_ready) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  uint32_t team_wgs = 0;
  *hypotheses_per_launch = batch_width(ctx, &team_wgs);
  return VGICP_OK;
}
}  // extern "C"
