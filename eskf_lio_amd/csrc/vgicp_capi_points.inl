// vgicp_capi_points.inl — part of vgicp_capi.hip.
// vgicp_points_resident (include/vgicp_hip_points.h) behind its entry point in libvgicp_hip_points.so: the refusals
// (plan_points, vgicp_points_plan.h), the call frame (vgicp_capi_resident.inl), the launches with their one
// synchronisation, the delivery.  Reads the context; writes only the report's own storage (d_points, h_points) and the arena.
namespace {
// ctx->d_points carved for `cap` points: the four planes, the sort's two (key, index) buffers and its splitters, the
// counters.  Everything at a 256-byte boundary.
struct PointsLayout {
  size_t d2, sq_error, weight, status, keys_a, keys_b, idx_a, idx_b, split, counters, total;
  explicit PointsLayout(size_t cap) {
    StageLayout lay;
    d2 = lay.take(cap * sizeof(double));
    sq_error = lay.take(cap * sizeof(double));
    weight = lay.take(cap * sizeof(double));
    status = lay.take(cap);
    keys_a = lay.take(cap * sizeof(unsigned long long));
    keys_b = lay.take(cap * sizeof(unsigned long long));
    idx_a = lay.take(cap * sizeof(uint32_t));
    idx_b = lay.take(cap * sizeof(uint32_t));
    split = lay.take(sort_keys64_scratch_bytes((uint32_t)cap));
    counters = lay.take(kPointCounters * sizeof(uint32_t));
    total = lay.total;
  }
};
template <class T> T* points_at(const vgicp_ctx* ctx, size_t offset) { return reinterpret_cast<T*>(ctx->d_points.get() + offset); }

PointsFacts points_facts(const vgicp_ctx* ctx, const double* pose, size_t capacity, bool any_array, size_t n_quantiles,
                         const double* q, const vgicp_point_summary* summary) {
  PointsFacts f;
  static_cast<ResidentFacts&>(f) = resident_facts(ctx);
  f.pose = pose != nullptr;
  f.pose_finite = !pose || first_not_finite(pose, 16) == 16;
  f.n_quantiles = n_quantiles;
  f.q = q != nullptr;
  f.summary = summary != nullptr;
  if (q && n_quantiles <= kPointQuantilesMax)
    for (size_t j = 0; j < n_quantiles; ++j) f.q_in_range = f.q_in_range && q[j] >= 0.0 && q[j] <= 1.0;
  f.any_array = any_array;
  f.capacity = capacity;
  return f;
}
}  // namespace

namespace vgicp_internal {
int points_resident(vgicp_ctx* ctx, const double pose[16], size_t capacity, double* d2, double* sq_error, double* weight,
                    uint8_t* status, size_t n_quantiles, const double* q, vgicp_point_summary* summary,
                    vgicp_point_stats* stats) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  PointsFacts facts = points_facts(ctx, pose, capacity, d2 || sq_error || weight || status, n_quantiles, q, summary);
  PointsVerdict v = plan_points(facts);
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  const TimedSpan span;
  VG_RC(settle_resident(ctx, &facts));   // the capacity check and the launch geometry are made from the kept count
  v = plan_points(facts);
  if (v.status != VGICP_OK) {
    if (v.sets_points && summary) summary->points = ctx->n;
    return fail(ctx, v.status, v.text);
  }

  const uint32_t n = ctx->n;
  // scratch: sized from the scan's capacity, so that scans of one size allocate once; never shared with the preparation's
  const size_t cap = std::max<size_t>(ctx->scan_capacity, n);
  if (!ctx->d_points || ctx->points_capacity < cap) {
    ctx->points_capacity = 0;
    VG_HIP(ctx, ctx->d_points.alloc(PointsLayout(cap).total));
    ctx->points_capacity = cap;
  }
  if (!ctx->h_points) VG_HIP(ctx, ctx->h_points.alloc_mapped(kPointResultWords * sizeof(unsigned long long)));
  const PointsLayout lay(ctx->points_capacity);

  PointArgs a;
  std::memset(&a, 0, sizeof a);
  static_cast<PoseView&>(a) = pose_view(ctx, pose);   // settled: n is the resident scan's size
  const RobustArgs robust = robust_args(ctx);
  a.robust_kernel = robust.kernel;
  a.robust_scale2 = robust.scale2;
  a.robust_gate = robust.gate;
  a.d2 = d2 ? points_at<double>(ctx, lay.d2) : nullptr;
  a.sq_error = sq_error ? points_at<double>(ctx, lay.sq_error) : nullptr;
  a.weight = weight ? points_at<double>(ctx, lay.weight) : nullptr;
  a.status = status ? points_at<uint8_t>(ctx, lay.status) : nullptr;
  const bool ranks = n_quantiles > 0 && n > 0;
  a.keys = ranks ? points_at<unsigned long long>(ctx, lay.keys_a) : nullptr;
  a.idx = ranks ? points_at<uint32_t>(ctx, lay.idx_a) : nullptr;
  a.counters = points_at<uint32_t>(ctx, lay.counters);

  PointPickArgs pick;
  std::memset(&pick, 0, sizeof pick);
  pick.sorted = points_at<unsigned long long>(ctx, lay.keys_b);
  pick.counters = a.counters;
  pick.n = n;
  pick.n_quantiles = (uint32_t)n_quantiles;
  for (size_t j = 0; j < n_quantiles; ++j) pick.q[j] = q[j];
  pick.out = ctx->h_points.dev();

  int launches = n ? 2 : 1;
  VG_RC(span.begin(ctx));
  VG_HIP(ctx, hipMemsetAsync(a.counters, 0, kPointCounters * sizeof(uint32_t), ctx->stream));
  VG_HIP(ctx, launch_point_terms(ctx->stream, a));
  if (ranks) {
    uint32_t sort_launches = 0;
    VG_HIP(ctx, launch_sort_keys64(ctx->stream, a.keys, a.idx, points_at<unsigned long long>(ctx, lay.keys_b),
                                   points_at<uint32_t>(ctx, lay.idx_b), points_at<void>(ctx, lay.split), n, &sort_launches));
    launches += (int)sort_launches;
  }
  VG_HIP(ctx, launch_point_pick(ctx->stream, pick));
  VG_RC(span.end(ctx));
  // the arrays: through the arena, the runtime never sees the caller's pages
  arena_reset(ctx);
  if (n) {
    if (d2) VG_RC(user_d2h(ctx, d2, a.d2, (size_t)n * sizeof(double)));
    if (sq_error) VG_RC(user_d2h(ctx, sq_error, a.sq_error, (size_t)n * sizeof(double)));
    if (weight) VG_RC(user_d2h(ctx, weight, a.weight, (size_t)n * sizeof(double)));
    if (status) VG_RC(user_d2h(ctx, status, a.status, (size_t)n));
  }
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  user_copies_finish(ctx);
  if (summary) {
    const unsigned long long* r = ctx->h_points;
    summary->points = n;
    summary->matched = r[0];
    summary->counted = r[1];
    summary->negative = r[2];
    summary->not_finite = r[3];
    for (size_t j = 0; j < n_quantiles; ++j) summary->quantile[j] = point_key_value(r[kPointCounters + j]);
  }
  if (stats) {
    VG_RC(span.device_seconds(ctx, &stats->device_seconds));
    stats->launches = launches;
    stats->reserved = 0;
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}
}  // namespace vgicp_internal
