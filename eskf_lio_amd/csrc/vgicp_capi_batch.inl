// vgicp_capi_batch.inl — part of vgicp_capi.hip.
// vgicp_align_resident_batch / vgicp_align_batch_width (include/vgicp_hip_batch.h): the plan (plan_batch,
// vgicp_resident_plan.h), the call frame (vgicp_capi_resident.inl), the launches with their one synchronisation, and the k
// single aligns in a row.  Whether a batch runs as teams, and how
// wide: plan_align / team_width (vgicp_align_plan.h).
namespace {
AlignState* batch_state(const vgicp_ctx* ctx, size_t h) {
  return reinterpret_cast<AlignState*>(ctx->h_batch + h * (size_t)kBatchSlotRows * kSlots);
}

void batch_report(size_t h, int max_it, const AlignState* st, const double* log, vgicp_batch_stats* stats) {
  if (!stats) return;
  if (stats->iterations) stats->iterations[h] = st->iteration;
  if (stats->converged) stats->converged[h] = st->converged;
  report_rows(st->iteration, log, stats->corr_count ? stats->corr_count + h * (size_t)max_it : nullptr,
              stats->normal_eq ? stats->normal_eq + h * (size_t)max_it * kNormalEq : nullptr);
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
  persistent_args_common(ctx, params, &a);   // n is settled: the kept count; one sequence number for the whole call
  a.rows = ctx->d_batch_exchange;
  a.parts = ctx->d_batch_exchange + team_rows_words();
  a.spin_limit = ctx->persist_spin_limit;
  a.round0 = 0;   // every launch starts from unset words
  a.world = 1;
  a.prefetch_margin = ctx->prefetch_margin;   // one point per thread, no memo, no stash: as the single launch has it
  TeamArgs t;
  std::memset(&t, 0, sizeof t);
  t.team_wgs = team_wgs;
  t.folder_rows = (team_wgs + kFolders - 1) / kFolders;
  t.slot_words = (uint32_t)slot_words;
  t.abort_word = reinterpret_cast<uint32_t*>(ctx->h_batch.dev() + (size_t)VGICP_BATCH_MAX * slot_words);
  *abort_host = 0;
  for (size_t h = 0; h < k; ++h) {
    AlignState* st = batch_state(ctx, h);
    st->seq = 0;
    st->outcome = kOutcomeNone;
  }
  const size_t exchange_bytes = (team_rows_words() + team_parts_words()) * 8;
  int launches = 0;
  VG_RC(TimedSpan::begin(ctx));
  for (size_t h0 = 0; h0 < k; h0 += width, ++launches) {
    t.teams = (uint32_t)std::min<size_t>(width, k - h0);
    for (uint32_t h = 0; h < t.teams; ++h) pose_to_state(guesses + 16 * (h0 + h), t.pose0[h]);
    a.state = reinterpret_cast<AlignState*>(ctx->h_batch.dev() + h0 * slot_words);
    a.log = ctx->h_batch.dev() + h0 * slot_words + kSlots;
    // T, and with it the owner of every exchange word, changes with the scan, and teams end in different rounds: every
    // launch starts from words that are unset throughout (0xFF bytes = kRowUnset)
    VG_HIP(ctx, hipMemsetAsync(ctx->d_batch_exchange, 0xFF, exchange_bytes, ctx->stream));
    VG_HIP(ctx, launch_persistent_teams(ctx->stream, a, t, ctx->persist_grid));
  }
  VG_RC(TimedSpan::end(ctx));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double device_seconds = 0.0;
  VG_RC(TimedSpan::device_seconds(ctx, &device_seconds));
  ctx->persistent_launches += (uint64_t)launches;
  // accepted only if every team's echo is there and nobody gave up: the ONE abort word speaks for every hypothesis
  bool committed = true;
  for (size_t h = 0; h < k && committed; ++h) committed = launch_committed(*batch_state(ctx, h), a.seq, *abort_host);
  if (!committed) {
    count_fallback(ctx, "batched align launch gave up waiting for a workgroup", "this batch and ");
    return VGICP_OK;
  }
  *ran = true;
  for (size_t h = 0; h < k; ++h) {
    const AlignState* st = batch_state(ctx, h);
    batch_report(h, max_it, st, ctx->h_batch + h * slot_words + kSlots, stats);
    const int status = report_pose(ctx, *st, out_poses + 16 * h);
    if (stats && stats->status) stats->status[h] = status;
    if (status != VGICP_OK && *first_bad == VGICP_OK) *first_bad = status;
  }
  if (stats) {
    stats->hypotheses_per_launch = (int32_t)std::min<size_t>(width, k);
    stats->launches = launches;
    stats->device_seconds = device_seconds;
  }
  return VGICP_OK;
}
}  // namespace

// The k aligns one after another through the single call's own paths (also the multi-device forward); loop_only: on the
// launch-per-round loop (align_on_loop), which touches neither cool-down nor counters.  Any status but VGICP_OK /
// VGICP_ERR_DEGENERATE ends the batch.
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
    const int rc = loop_only ? align_on_loop(ctx, guesses + 16 * h, params, out_poses + 16 * h, &st, now_seconds())
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
  BatchFacts f;
  f.ctx = ctx != nullptr, f.k = k, f.guesses = guesses != nullptr, f.out_poses = out_poses != nullptr, f.params = params != nullptr;
  if (params) f.max_iteration = params->max_iteration;
  if (ctx) f.multi = ctx->multi != nullptr, f.at = resident_facts(ctx);
  const ResidentVerdict v = plan_batch(f);
  VG_RC(refuse(ctx, v));
  const TimedSpan span;
  int first_bad = VGICP_OK;
  int rc = VGICP_OK;
  if (v.forward) {
    rc = vgicp_multi_api::align_resident_batch(ctx, k, guesses, params, out_poses, stats, &first_bad);
    if (rc != VGICP_OK) return rc;
    if (stats) stats->seconds = span.seconds();
    return (stats && stats->status) ? VGICP_OK : first_bad;
  }
  VG_RC(settle_resident(ctx, &f.at));   // the team layout is made from the kept count
  VG_RC(refuse(ctx, plan_batch(f)));
  const AlignPlan plan = plan_align(align_facts(ctx, params, AlignCall::Batch, ctx->n, k));
  bool ran = false;
  if (plan.width < 2) {
    rc = vgicp_internal::align_batch_sequential(ctx, k, guesses, params, out_poses, stats, /*loop_only=*/false, &first_bad);
  } else {
    // inside the cool-down no launch is attempted and nothing is counted: k aligns on the loop, k aligns of cool-down
    ctx->persistent_cooldown -= plan.cooldown_drop;
    if (plan.path == AlignPath::Teams)
      rc = run_batch_teams(ctx, k, guesses, params, plan.width, plan.team_wgs, out_poses, stats, &first_bad, &ran);
    if (rc == VGICP_OK && !ran)
      rc = vgicp_internal::align_batch_sequential(ctx, k, guesses, params, out_poses, stats, /*loop_only=*/true, &first_bad);
  }
  if (rc != VGICP_OK) return rc;
  if (stats) stats->seconds = span.seconds();
  return (stats && stats->status) ? VGICP_OK : first_bad;
}

int vgicp_align_batch_width(vgicp_ctx* ctx, size_t* hypotheses_per_launch) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (!hypotheses_per_launch) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "hypotheses_per_launch is NULL");
  *hypotheses_per_launch = 1;
  if (ctx->multi) return vgicp_multi_api::align_batch_width(ctx, hypotheses_per_launch);
  VG_RC(settle(ctx));
  if (!ctx->scan_ready) return fail(ctx, VGICP_ERR_NOT_READY, kNoScanText);
  uint32_t team_wgs = 0;
  *hypotheses_per_launch = team_width(align_facts(ctx, nullptr, AlignCall::Batch, ctx->n), &team_wgs);
  return VGICP_OK;
}
}  // extern "C"
