// vgicp_capi_evaluate.inl — part of vgicp_capi.hip.
// vgicp_evaluate_resident (include/vgicp_hip_evaluate.h): the plan (plan_evaluate, vgicp_resident_plan.h), the call frame
// (vgicp_capi_resident.inl), the launch pairs with their one synchronisation, the report.  Reads the context; writes
// only the evaluation's own storage (d_eval_rows, h_eval).
extern "C" {

int vgicp_evaluate_resident(vgicp_ctx* ctx, size_t k, const double* poses, vgicp_evaluation* out, vgicp_eval_stats* stats) {
  EvaluateFacts f;
  f.ctx = ctx != nullptr, f.k = k, f.poses = poses != nullptr, f.out = out != nullptr;
  const bool readable = poses && k >= 1 && k <= (size_t)VGICP_EVAL_MAX;   // what rules 2 and 3 ask comes first
  const size_t bad = readable ? first_not_finite(poses, 16 * k) : 16 * k;
  if (bad < 16 * k) f.bad_pose = (int64_t)(bad / 16);
  if (ctx) f.at = resident_facts(ctx);
  const ResidentVerdict v = plan_evaluate(f);
  if (v.rule == 4) return fail(ctx, v.status, "pose " + std::to_string(f.bad_pose) + v.text);
  VG_RC(refuse(ctx, v));
  const TimedSpan span;
  VG_RC(settle_resident(ctx, &f.at));   // the launch geometry is made from the kept count
  VG_RC(refuse(ctx, plan_evaluate(f)));

  const uint32_t rows = iterate_grid(ctx->n, 512);   // workgroups per pose: the grid of the loop's 512-thread launch
  const size_t per_launch = std::min<size_t>(VGICP_EVAL_MAX, (size_t)kEvalRowBudget / rows);
  double* h_poses = ctx->h_eval + (size_t)VGICP_EVAL_MAX * kSlots;
  for (size_t h = 0; h < k; ++h) pose_to_state(poses + 16 * h, h_poses + 12 * h);
  EvalArgs a;
  std::memset(&a, 0, sizeof a);
  static_cast<ResidentView&>(a) = resident_view(ctx);
  a.rows = ctx->d_eval_rows;
  set_symmetry(ctx, &a);
  int launches = 0;
  VG_RC(span.begin(ctx));
  for (size_t h0 = 0; h0 < k; h0 += per_launch) {
    const uint32_t m = (uint32_t)std::min<size_t>(per_launch, k - h0);
    a.poses = ctx->h_eval.dev() + (size_t)VGICP_EVAL_MAX * kSlots + 12 * h0;
    // stream order: this pair's rows are written after the previous pair's fold has read its own
    VG_HIP(ctx, launch_evaluate(ctx->stream, a, rows, m));
    VG_HIP(ctx, launch_evaluate_fold(ctx->stream, ctx->d_eval_rows, rows, m, ctx->h_eval.dev() + h0 * kSlots));
    launches += 2;
  }
  VG_RC(span.end(ctx));
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
    VG_RC(span.device_seconds(ctx, &stats->device_seconds));
    stats->launches = launches;
    stats->poses_per_launch = (int32_t)per_launch;
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}
}  // extern "C"
