// vgicp_capi_map_rays.inl — part of vgicp_capi.hip.
// The ray report (include/vgicp_hip_map_rays.h) behind its entry point in libvgicp_hip_map_rays.so: the refusals
// (plan_rays, vgicp_map_plan.h), the settling, the confirmation bitmap, the groups of poses (per group: a clear and the
// two launches of launch_map_rays, vgicp_mapupdate.hip) and the delivery.  Read-only: nothing of the map's or the scan's
// bookkeeping is touched.
namespace {
static_assert(sizeof(vgicp_ray_counts) == kRayCountWords * sizeof(unsigned long long), "the kernel's counter block is vgicp_ray_counts");
static_assert(kRayMaxPoses == VGICP_RAYS_MAX_POSES, "vgicp_map_plan.h plans with the header's limit");
RayFacts ray_facts(const vgicp_ctx* ctx, const double* poses, size_t n_poses, const vgicp_ray_params* p,
                   const vgicp_ray_outputs* per_point) {
  RayFacts f;
  // as the carving entries: the first sub-context of a multi-device context answers rule 3; rule 11 then refuses it
  const vgicp_ctx* at = facts_of(ctx);
  static_cast<ResidentFacts&>(f) = resident_facts(at);
  f.several_devices = several_devices(ctx);
  f.pointers = poses != nullptr && p != nullptr;
  f.n_poses = n_poses;
  if (f.pointers && n_poses >= 1 && n_poses <= kRayMaxPoses) {
    f.entries_finite = first_not_finite(poses, 16 * n_poses) == 16 * n_poses && first_not_finite(p->origin, 3) == 3;
    f.margin = p->margin;
    f.beyond = p->beyond;
    f.max_range = p->max_range;
    f.stride = p->stride;
    f.reserved = p->reserved;
  }
  f.per_point = per_point && (per_point->status || per_point->range || per_point->hit_key || per_point->steps);
  f.voxel_size = at->voxel_size;
  return f;
}
// the bitmap of one group of poses, for the table as it is: made anew only when the slot count has changed
int ensure_ray_bits(vgicp_ctx* ctx) {
  if (ctx->d_ray_bits && ctx->ray_bits_slots == ctx->slots) return VGICP_OK;
  ctx->ray_bits_slots = 0;
  VG_HIP(ctx, ctx->d_ray_bits.alloc(ray_group_poses(ctx->slots) * ray_bitmap_bytes(ctx->slots)));
  ctx->ray_bits_slots = ctx->slots;
  return VGICP_OK;
}
}  // namespace

namespace vgicp_internal {
int rays_resident(vgicp_ctx* ctx, const double* poses, size_t n_poses, const vgicp_ray_params* params,
                  const vgicp_ray_outputs* per_point, vgicp_ray_counts* counts, vgicp_ray_stats* stats) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  const TimedSpan span;
  if (!several_devices(ctx)) VG_RC(settle(ctx));
  const RayVerdict v = plan_rays(ray_facts(ctx, poses, n_poses, params, per_point));
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  const uint64_t launches0 = g_kernel_launches;
  const size_t n = ctx->n;
  const bool launched = n != 0;
  const vgicp_ray_outputs want = per_point ? *per_point : vgicp_ray_outputs{nullptr, nullptr, nullptr, nullptr};
  const size_t count_bytes = n_poses * kRayCountWords * sizeof(unsigned long long);
  uint32_t groups = 0;
  if (launched) {
    VG_HIP(ctx, hipSetDevice(ctx->device));
    // device (d_stage) and page-locked (h_rays) memory of the call, laid out alike: poses, counts, the planes asked for
    StageLayout lay;
    const size_t o_poses = lay.take(n_poses * 12 * sizeof(double)), o_counts = lay.take(count_bytes);
    const size_t o_range = lay.take(want.range ? n * sizeof(double) : 0), o_keys = lay.take(want.hit_key ? n * 3 * sizeof(int32_t) : 0);
    const size_t o_steps = lay.take(want.steps ? n * sizeof(uint32_t) : 0), o_status = lay.take(want.status ? n : 0);
    VG_RC(ensure_stage(ctx, lay.total));
    if (lay.total > ctx->h_rays.bytes()) VG_HIP(ctx, ctx->h_rays.alloc(lay.total + lay.total / 2));
    VG_RC(ensure_ray_bits(ctx));
    char* h = ctx->h_rays;
    double* h_poses = reinterpret_cast<double*>(h + o_poses);
    for (size_t k = 0; k < n_poses; ++k) pose_to_state(poses + 16 * k, h_poses + 12 * k);

    RayArgs a;
    std::memset(&a, 0, sizeof a);
    a.table = ctx->table;
    a.slots = ctx->slots;
    a.voxel_size = ctx->voxel_size;
    a.points_aos = ctx->d_scan_aos;
    a.n = (uint32_t)n;
    a.stride = params->stride;
    for (int k = 0; k < 3; ++k) a.origin[k] = params->origin[k];
    a.margin = params->margin;
    a.beyond = params->beyond;
    a.max_range = params->max_range;
    a.bits = ctx->d_ray_bits;
    a.status = want.status ? stage_at<uint8_t>(ctx, o_status) : nullptr;
    a.range = want.range ? stage_at<double>(ctx, o_range) : nullptr;
    a.hit_key = want.hit_key ? stage_at<int32_t>(ctx, o_keys) : nullptr;
    a.steps = want.steps ? stage_at<uint32_t>(ctx, o_steps) : nullptr;
    double* d_poses = stage_at<double>(ctx, o_poses);
    unsigned long long* d_counts = stage_at<unsigned long long>(ctx, o_counts);
    VG_HIP(ctx, hipMemcpyAsync(d_poses, h_poses, n_poses * 12 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    VG_HIP(ctx, hipMemsetAsync(d_counts, 0, count_bytes, ctx->stream));
    const size_t per = (size_t)ray_group_poses(ctx->slots), bitmap = (size_t)ray_bitmap_bytes(ctx->slots);
    VG_RC(TimedSpan::begin(ctx));
    for (size_t first = 0; first < n_poses; first += per, ++groups) {   // no host round trip between groups
      a.n_poses = (uint32_t)std::min(per, n_poses - first);
      a.poses = d_poses + 12 * first;
      a.counts = d_counts + kRayCountWords * first;
      VG_HIP(ctx, hipMemsetAsync(ctx->d_ray_bits, 0, a.n_poses * bitmap, ctx->stream));
      VG_HIP(ctx, launch_map_rays(ctx->stream, a));
    }
    VG_RC(TimedSpan::end(ctx));
    VG_HIP(ctx, hipMemcpyAsync(h + o_counts, d_counts, count_bytes, hipMemcpyDeviceToHost, ctx->stream));
    // the planes asked for lie in one piece of both layouts, from the first of them to the end
    const size_t planes_at = want.range ? o_range : want.hit_key ? o_keys : want.steps ? o_steps : o_status;
    if (lay.total > planes_at)
      VG_HIP(ctx, hipMemcpyAsync(h + planes_at, stage_at<char>(ctx, planes_at), lay.total - planes_at, hipMemcpyDeviceToHost, ctx->stream));
    VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (counts) std::memcpy(counts, h + o_counts, count_bytes);
    if (want.status) std::memcpy(want.status, h + o_status, n);
    if (want.range) std::memcpy(want.range, h + o_range, n * sizeof(double));
    if (want.hit_key) std::memcpy(want.hit_key, h + o_keys, n * 3 * sizeof(int32_t));
    if (want.steps) std::memcpy(want.steps, h + o_steps, n * sizeof(uint32_t));
  } else if (counts) {
    std::memset(counts, 0, count_bytes);
  }
  if (stats) {
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    stats->groups = (int32_t)groups;
    stats->device_seconds = 0.0;   // nothing to do: no span was recorded
    if (launched) VG_RC(span.device_seconds(ctx, &stats->device_seconds));
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}
}  // namespace vgicp_internal
