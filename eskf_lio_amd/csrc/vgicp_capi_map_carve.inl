// vgicp_capi_map_carve.inl — part of vgicp_capi.hip.
// Free-space carving (include/vgicp_hip_map_carve.h) behind its entry points in libvgicp_hip_map_carve.so: the refusals
// (plan_carve, vgicp_map_plan.h), the settling, the two launches (launch_map_carve, vgicp_mapupdate.hip) and the
// removal's bookkeeping — finish_removal's arithmetic at once, or at the next settle() for the deferred form.
namespace {
CarveFacts carve_facts(const vgicp_ctx* ctx, const double* transform, const vgicp_carve_params* p) {
  CarveFacts f;
  // as the gated entries: a multi-device context keeps its map and scan in its sub-contexts, so the first of them
  // answers rule 3; rule 9 then refuses the context for what it is
  const vgicp_ctx* at = facts_of(ctx);
  static_cast<ResidentFacts&>(f) = resident_facts(at);
  f.several_devices = several_devices(ctx);
  f.pointers = transform != nullptr && p != nullptr;
  if (f.pointers) {
    f.entries_finite = first_not_finite(transform, 16) == 16 && first_not_finite(p->origin, 3) == 3;
    f.margin = p->margin;
    f.max_range = p->max_range;
    f.min_hits = p->min_hits;
    f.stride = p->stride;
  }
  f.voxel_size = at->voxel_size;
  return f;
}
// what both forms launch with: everything but where the counts go
CarveArgs carve_args(const vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params& p) {
  CarveArgs a;
  std::memset(&a, 0, sizeof a);
  a.table = ctx->table;
  a.slots = ctx->slots;
  a.voxel_size = ctx->voxel_size;
  a.points_aos = ctx->d_scan_aos;
  a.n = ctx->n;
  a.stride = p.stride;
  a.min_hits = p.min_hits;
  pose_to_state(transform, a.pose);
  for (int k = 0; k < 3; ++k) a.origin[k] = p.origin[k];
  a.margin = p.margin;
  a.max_range = p.max_range;
  return a;
}
// words of the synchronous call's counter block (staging area, zeroed in front of the launches): removed, touched,
// shielded, rays, visits (64 bits at word 4)
constexpr int kCarveCallWords = 8;
}  // namespace

namespace vgicp_internal {
int map_carve_resident(vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params* params, size_t capacity,
                       int32_t* removed_keys, size_t* removed, vgicp_carve_stats* stats) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  const TimedSpan span;
  if (!several_devices(ctx)) VG_RC(settle(ctx));
  const CarveVerdict v = plan_carve(carve_facts(ctx, transform, params));
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  const uint64_t launches0 = g_kernel_launches;
  uint32_t counts[kCarveCallWords] = {0};
  const bool launched = ctx->n != 0;
  if (launched) {
    VG_HIP(ctx, hipSetDevice(ctx->device));
    // the key list cannot be longer than the map (or than the caller's room)
    const size_t room = removed_keys ? std::min<size_t>(capacity, ctx->voxels) : 0;
    StageLayout lay;
    const size_t o_counts = lay.take(kCarveCallWords * sizeof(uint32_t)), o_keys = lay.take(room * 3 * sizeof(int32_t));
    VG_RC(ensure_stage(ctx, lay.total));
    if (room > ctx->carve_keys_capacity) {
      ctx->carve_keys_capacity = 0;
      VG_HIP(ctx, ctx->h_carve_keys.alloc((room + room / 2) * 3 * sizeof(int32_t)));
      ctx->carve_keys_capacity = room + room / 2;
    }
    uint32_t* d_counts = stage_at<uint32_t>(ctx, o_counts);
    CarveArgs a = carve_args(ctx, transform, *params);
    a.removed = d_counts;
    a.touched = d_counts + 1;
    a.shielded = d_counts + 2;
    a.rays = d_counts + 3;
    a.visits = reinterpret_cast<unsigned long long*>(d_counts + 4);
    a.keys = room ? stage_at<int32_t>(ctx, o_keys) : nullptr;
    a.keys_capacity = (uint32_t)std::min<size_t>(room, 0xFFFFFFFFu);
    VG_HIP(ctx, hipMemsetAsync(d_counts, 0, kCarveCallWords * sizeof(uint32_t), ctx->stream));
    ++ctx->map_version;   // the dense copy is out of date
    VG_RC(TimedSpan::begin(ctx));
    VG_HIP(ctx, launch_map_carve(ctx->stream, a));
    VG_RC(TimedSpan::end(ctx));
    VG_HIP(ctx, hipMemcpyAsync(ctx->h_counters, d_counts, kCarveCallWords * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (room) VG_HIP(ctx, hipMemcpyAsync(ctx->h_carve_keys, a.keys, room * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < kCarveCallWords; ++k) counts[k] = ctx->h_counters[k];
    // finish_removal's arithmetic
    ctx->voxels -= counts[0];
    ctx->tombstones += counts[0];
    ctx->carve_removed += counts[0];
    ctx->carve_rays += counts[3];
    if (room) std::memcpy(removed_keys, ctx->h_carve_keys, std::min<size_t>(room, counts[0]) * 3 * sizeof(int32_t));
  }
  if (removed) *removed = counts[0];
  if (stats) {
    stats->removed = counts[0];
    stats->touched = counts[1];
    stats->shielded = counts[2];
    stats->rays = counts[3];
    stats->visits = (uint64_t)counts[4] | ((uint64_t)counts[5] << 32);
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    stats->reserved = 0;
    stats->device_seconds = 0.0;   // nothing to do: no span was recorded
    if (launched) VG_RC(span.device_seconds(ctx, &stats->device_seconds));
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}

int map_carve_resident_async(vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params* params) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  // as vgicp_map_insert_resident_async: nothing this entry refuses depends on the scan's size
  const CarveVerdict v = plan_carve(carve_facts(ctx, transform, params));
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  VG_RC(settle_if_pending(ctx));   // (a carve that is pending on its own is not waited for: its totals keep running)
  if (ctx->n == 0) return VGICP_OK;
  VG_HIP(ctx, hipSetDevice(ctx->device));
  CarveArgs a = carve_args(ctx, transform, *params);
  a.rays = ctx->d_ins_counters + kCarveRaysWord;
  a.removed = ctx->d_ins_counters + kCarveRemovedWord;
  ++ctx->map_version;
  VG_HIP(ctx, launch_map_carve(ctx->stream, a));
  ctx->carve_pending = true;
  ctx->ins_copy_enqueued = false;   // the next preparation's counter copy carries the totals (or settle() fetches them)
  return VGICP_OK;
}

int map_carve_totals(vgicp_ctx* ctx, uint64_t* rays, uint64_t* removed) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (!several_devices(ctx)) VG_RC(settle(ctx));
  if (rays) *rays = ctx->carve_rays;
  if (removed) *removed = ctx->carve_removed;
  return VGICP_OK;
}
}  // namespace vgicp_internal
