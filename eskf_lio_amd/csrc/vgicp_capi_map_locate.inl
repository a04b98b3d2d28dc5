// vgicp_capi_map_locate.inl — part of vgicp_capi.hip.
// Locate (include/vgicp_hip_map_locate.h) behind its entry point in libvgicp_hip_map_locate.so: the refusals
// (plan_locate, vgicp_locate_plan.h), the settling, the level's lazy rebuild (ensure_levels), the clear and the two
// launches of launch_locate (vgicp_levels.hip), the delivery.  Read-only: nothing of the map's, the scan's or an
// align's bookkeeping is touched; the call's storage is its own.
namespace {
static_assert(VGICP_LOCATE_MAX_POSES == VGICP_EVAL_MAX, "a fan of guesses is scored and located alike");
// d_locate: the poses, the skipped counts, the plane (the two that are cleared lie together).  h_locate: the poses, the
// bests, the plane.  Both of one size, whatever the call asks.
struct LocateLayout {
  static constexpr size_t poses = 0, pose_bytes = (size_t)VGICP_LOCATE_MAX_POSES * 16 * sizeof(double);
  static constexpr size_t plane_bytes = (size_t)VGICP_LOCATE_MAX_POSES * VGICP_LOCATE_MAX_CELLS * sizeof(uint32_t);
  static constexpr size_t d_skipped = pose_bytes, d_plane = d_skipped + VGICP_LOCATE_MAX_POSES * sizeof(uint32_t);
  static constexpr size_t d_total = d_plane + plane_bytes;
  static constexpr size_t h_best = pose_bytes, h_plane = h_best + VGICP_LOCATE_MAX_POSES * sizeof(vgicp_locate_best);
  static constexpr size_t h_total = h_plane + plane_bytes;
};
LocateFacts locate_facts(const vgicp_ctx* ctx, const double* poses, size_t k, const vgicp_locate_params* p, const vgicp_locate_best* best) {
  LocateFacts f;
  f.ctx = ctx != nullptr;
  f.pointers = poses && p && best;
  f.k = k;
  if (p) {
    f.level = p->level;
    for (int a = 0; a < 3; ++a) f.window[a] = p->window[a];
    f.stride = p->stride;
  }
  if (poses && k >= 1 && k <= (size_t)VGICP_LOCATE_MAX_POSES) f.poses_finite = first_not_finite(poses, 16 * k) == 16 * k;
  if (ctx) {
    f.requested = ctx->levels_requested;
    // as the levels' entries: a multi-device context keeps its map and scan in its sub-contexts; rule 5 refuses it first
    f.at = resident_facts(facts_of(ctx));
    f.at.several_devices = several_devices(ctx);
  }
  return f;
}
}  // namespace

namespace vgicp_internal {
int locate_resident(vgicp_ctx* ctx, const double* poses, size_t k, const vgicp_locate_params* params, vgicp_locate_best* best,
                    uint32_t* hits, vgicp_locate_stats* stats) {
  LocateFacts f = locate_facts(ctx, poses, k, params, best);
  VG_RC(refuse(ctx, plan_locate(f)));
  const TimedSpan span;
  VG_RC(settle_resident(ctx, &f.at));   // the levels are sized from the map's voxel count, the launch from the scan's
  VG_RC(refuse(ctx, plan_locate(f)));
  if (!ctx->d_locate) {
    VG_HIP(ctx, ctx->d_locate.alloc(LocateLayout::d_total));
    VG_HIP(ctx, ctx->h_locate.alloc_mapped(LocateLayout::h_total));
  }
  const uint64_t launches0 = g_kernel_launches;
  const int level = params->level;
  if (level > 0) VG_RC(ensure_levels(ctx));   // enqueued in front of the score launch; its counts ride on this call's wait

  LocateArgs a;
  std::memset(&a, 0, sizeof a);
  a.table = level == 0 ? ctx->table.get() : ctx->level[level - 1].table.get();
  a.mask = (uint32_t)((level == 0 ? ctx->slots : ctx->level[level - 1].slots) - 1);
  a.voxel_size = level_voxel_size(ctx->voxel_size, level);
  a.points_aos = ctx->d_scan_aos;
  a.n = ctx->n;
  a.stride = params->stride;
  a.participants = (uint32_t)locate_participants(ctx->n, a.stride);
  int64_t w[3];
  for (int e = 0; e < 3; ++e) w[e] = a.window[e] = params->window[e];
  a.cells = (uint32_t)locate_cells(w);
  a.poses = reinterpret_cast<const double*>(ctx->d_locate + LocateLayout::poses);
  a.skipped = reinterpret_cast<uint32_t*>(ctx->d_locate + LocateLayout::d_skipped);
  a.plane = reinterpret_cast<uint32_t*>(ctx->d_locate + LocateLayout::d_plane);

  const size_t plane_bytes = k * a.cells * sizeof(uint32_t);
  std::memcpy(ctx->h_locate + LocateLayout::poses, poses, k * 16 * sizeof(double));
  VG_HIP(ctx, hipMemcpyAsync(ctx->d_locate + LocateLayout::poses, ctx->h_locate + LocateLayout::poses, k * 16 * sizeof(double),
                             hipMemcpyHostToDevice, ctx->stream));
  VG_RC(TimedSpan::begin(ctx));
  // ONE clear: the skipped counts and the plane lie together
  VG_HIP(ctx, hipMemsetAsync(a.skipped, 0, LocateLayout::d_plane - LocateLayout::d_skipped + plane_bytes, ctx->stream));
  VG_HIP(ctx, launch_locate(ctx->stream, a, (uint32_t)k, ctx->h_locate.dev() + LocateLayout::h_best));
  VG_RC(TimedSpan::end(ctx));
  if (hits)
    VG_HIP(ctx, hipMemcpyAsync(ctx->h_locate + LocateLayout::h_plane, a.plane, plane_bytes, hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  VG_RC(note_level_counts(ctx));
  std::memcpy(best, ctx->h_locate + LocateLayout::h_best, k * sizeof(vgicp_locate_best));
  if (hits) std::memcpy(hits, ctx->h_locate + LocateLayout::h_plane, plane_bytes);
  if (stats) {
    stats->cells = (int32_t)a.cells;
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    VG_RC(span.device_seconds(ctx, &stats->device_seconds));
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}
}  // namespace vgicp_internal
