// vgicp_capi_map_submap.inl — part of vgicp_capi.hip.
// Submap as scan (include/vgicp_hip_map_submap.h) behind its entry points in libvgicp_hip_map_submap.so: the refusals
// (plan_submap, vgicp_submap_plan.h), the settling of BOTH contexts, the level's lazy rebuild (ensure_levels), the wait of
// dst's stream for src's, the three launches of launch_submap (vgicp_mapupdate.hip), the one synchronisation and the
// bookkeeping of a new resident scan (begin_scan, as an upload's).
namespace {
SubmapFacts submap_facts(const vgicp_ctx* dst, const vgicp_ctx* src, const vgicp_submap_params* p) {
  SubmapFacts f;
  f.dst = dst != nullptr;
  f.src = src != nullptr;
  f.params = p != nullptr;
  if (!dst || !src || !p) return f;
  f.several_devices = several_devices(dst) || several_devices(src);
  f.same_device = dst->device == src->device;
  f.reserved = p->reserved;
  f.level = p->level;
  f.requested = src->levels_requested;
  f.center_finite = first_not_finite(p->center, 3) == 3;
  f.frame_finite = first_not_finite(p->frame, 16) == 16;
  f.radius = p->radius;
  f.src_has_map = src->table != nullptr;
  return f;
}
// grow-only; what the old buffers held is void by then (begin_scan follows)
int ensure_submap(vgicp_ctx* dst, uint64_t slots, size_t points) {
  if (!dst->h_submap) {
    VG_HIP(dst, dst->h_submap.alloc_mapped(4 * sizeof(unsigned long long)));
    std::memset(dst->h_submap, 0, 4 * sizeof(unsigned long long));
  }
  const size_t work = (size_t)submap_work_bytes(slots);
  if (work > dst->d_submap_work.bytes()) VG_HIP(dst, dst->d_submap_work.alloc(work));
  if (points > dst->submap_capacity || !dst->d_submap_keys) {
    dst->submap_capacity = 0;
    dst->submap_generation = 0;
    const size_t cap = std::max<size_t>(points + points / 4, 1024);
    VG_HIP(dst, dst->d_submap_keys.alloc(cap * (sizeof(uint64_t) + 3 * sizeof(int32_t))));
    dst->submap_capacity = cap;
  }
  return VGICP_OK;
}
}  // namespace

namespace vgicp_internal {
int scan_from_map(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_submap_params* params, vgicp_submap_stats* stats) {
  SubmapFacts f = submap_facts(dst, src, params);
  VG_RC(refuse(dst, plan_submap(f)));
  const TimedSpan span;
  VG_HIP(dst, hipSetDevice(dst->device));
  VG_RC(settle(src));
  if (dst != src) VG_RC(settle(dst));
  const uint64_t launches0 = g_kernel_launches;
  const int level = params->level;
  // enqueued on src's stream in front of the event below; the level's count rides on this call's wait.  Until it is here,
  // the map's own voxel count bounds it: a level has at most as many voxels as the one below
  if (level > 0) VG_RC(ensure_levels(src));
  f.settled = true;
  f.voxels = level == 0 || src->level_counts_pending ? src->voxels : src->level[level - 1].voxels;
  VG_RC(refuse(dst, plan_submap(f)));
  const uint64_t slots = level == 0 ? src->slots : src->level[level - 1].slots;
  const size_t upper = (size_t)f.voxels;
  if (upper > 0) VG_RC(ensure_submap(dst, slots, upper));
  if (upper > 0 && dst != src) {
    if (!src->ev_submap) VG_HIP(dst, src->ev_submap.create(false));
    VG_HIP(dst, hipEventRecord(src->ev_submap, src->stream));
    VG_HIP(dst, hipStreamWaitEvent(dst->stream, src->ev_submap, 0));
  }
  // from here on dst's resident scan is replaced
  VG_RC(begin_scan(dst, upper, 0.0, false));
  dst->n = 0;
  dst->scan_sym_known = false;
  dst->submap_generation = 0;
  unsigned long long totals[3] = {0ull, 0ull, 0ull};
  if (upper > 0) {
    SubmapArgs a;
    std::memset(&a, 0, sizeof a);
    a.table = level == 0 ? src->table.get() : src->level[level - 1].table.get();
    a.slots = slots;
    a.voxel_size = level_voxel_size(src->voxel_size, level);
    for (int e = 0; e < 3; ++e) a.center[e] = params->center[e];
    a.radius = params->radius;
    a.min_count = params->min_count;
    pose_to_state(params->frame, a.pose);
    a.groups = submap_groups(slots);
    char* work = dst->d_submap_work;
    a.ballots = reinterpret_cast<unsigned long long*>(work);
    a.group_counts = reinterpret_cast<uint32_t*>(work + (size_t)a.groups * kSubmapGroupWords * 8);
    a.totals = reinterpret_cast<unsigned long long*>(work + submap_work_bytes(slots) - 4 * 8);
    a.capacity = (uint32_t)std::min<uint64_t>({(uint64_t)dst->scan_capacity, (uint64_t)dst->submap_capacity, kScanPointsMax});
    a.aos_points = dst->d_scan_aos;
    a.aos_covs = dst->d_scan_aos + 3 * dst->scan_capacity;
    a.planes = dst->d_scan;
    a.stride = dst->stride;
    a.counts = reinterpret_cast<unsigned long long*>(dst->d_submap_keys.get());
    a.keys = reinterpret_cast<int32_t*>(dst->d_submap_keys + dst->submap_capacity * sizeof(uint64_t));
    VG_RC(TimedSpan::begin(dst));
    VG_HIP(dst, launch_submap(dst->stream, a, dst->h_submap.dev()));
    VG_RC(TimedSpan::end(dst));
    VG_HIP(dst, hipStreamSynchronize(dst->stream));   // THE synchronisation; src's work lies in front of dst's
    for (int k = 0; k < 3; ++k) totals[k] = dst->h_submap[k];
    if (totals[0] > a.capacity) return fail(dst, VGICP_ERR_HIP, "submap: more voxels selected than the source table was known to hold");
  } else if (level > 0 && src->level_counts_pending) {
    VG_HIP(dst, hipStreamSynchronize(src->stream));
  }
  if (level > 0) VG_RC(note_level_counts(src));
  dst->n = (uint32_t)totals[0];
  dst->scan_ready = totals[0] != 0;   // nothing selected: no resident scan
  dst->submap_generation = dst->scan_generation;
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->points = totals[0];
    stats->too_far = totals[1];
    stats->too_few = totals[2];
    stats->voxels = totals[0] + totals[1] + totals[2];
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    if (upper > 0) VG_RC(span.device_seconds(dst, &stats->device_seconds));
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}

int scan_from_map_keys(vgicp_ctx* dst, size_t capacity, int32_t* keys, uint64_t* counts, size_t* written) {
  if (!written) return fail(dst, VGICP_ERR_BAD_ARGUMENT, "written is NULL");
  if (several_devices(dst))
    return fail(dst, VGICP_ERR_BAD_ARGUMENT, "vgicp_scan_from_map_keys is not available on multi-device contexts, communicators "
                                             "and peer-connected contexts: the resident scan of a device is a shard there");
  if (dst->submap_generation == 0 || dst->submap_generation != dst->scan_generation)
    return fail(dst, VGICP_ERR_NOT_READY, "the resident scan is not one that vgicp_scan_from_map made");
  const size_t n = dst->n;
  *written = n;
  if (capacity < n) return fail(dst, VGICP_ERR_BAD_ARGUMENT, "capacity is below the scan's size");
  if (n == 0 || (!keys && !counts)) return VGICP_OK;
  VG_HIP(dst, hipSetDevice(dst->device));
  arena_reset(dst);
  if (counts) VG_RC(user_d2h(dst, counts, dst->d_submap_keys.get(), n * sizeof(uint64_t)));
  if (keys) VG_RC(user_d2h(dst, keys, dst->d_submap_keys + dst->submap_capacity * sizeof(uint64_t), n * 3 * sizeof(int32_t)));
  VG_HIP(dst, hipStreamSynchronize(dst->stream));
  user_copies_finish(dst);
  return VGICP_OK;
}
}  // namespace vgicp_internal
