// vgicp_capi_map_merge.inl — part of vgicp_capi.hip.
// Map merge (include/vgicp_hip_map_merge.h) behind its entry point in libvgicp_hip_map_merge.so: the refusals (plan_merge,
// vgicp_merge_plan.h), the settling of BOTH contexts, the destination table's growth (ensure_table, the insertion's), the
// scratch carved out of dst's staging area (merge_work), the wait of dst's stream for src's, the launches of
// launch_map_merge (vgicp_mapupdate.hip), the one synchronisation and the bookkeeping of a map update (begin_map_update,
// as an insertion's).
namespace {
uint64_t double_bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}
MergeFacts merge_facts(const vgicp_ctx* dst, const vgicp_ctx* src, const vgicp_merge_params* p) {
  MergeFacts f;
  f.dst = dst != nullptr;
  f.src = src != nullptr;
  f.params = p != nullptr;
  if (!dst || !src || !p) return f;
  f.several_devices = several_devices(dst) || several_devices(src);
  f.same_context = dst == src;
  f.same_device = dst->device == src->device;
  f.reserved = p->reserved;
  f.center_finite = first_not_finite(p->center, 3) == 3;
  f.frame_finite = first_not_finite(p->frame, 16) == 16;
  f.radius = p->radius;
  f.dst_has_map = dst->table != nullptr;
  f.src_has_map = src->table != nullptr;
  f.dst_voxel_bits = double_bits(dst->voxel_size);
  f.src_voxel_bits = double_bits(src->voxel_size);
  f.dst_raw = dst->raw_on;
  return f;
}
}  // namespace

namespace vgicp_internal {
int map_merge(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_merge_params* params, vgicp_merge_stats* stats) {
  MergeFacts f = merge_facts(dst, src, params);
  VG_RC(refuse(dst, plan_merge(f)));
  const TimedSpan span;
  VG_HIP(dst, hipSetDevice(dst->device));
  VG_RC(settle(src));
  VG_RC(settle(dst));
  const uint64_t launches0 = g_kernel_launches;
  f.settled = true;
  f.src_voxels = src->voxels;
  f.dst_slots = dst->slots;
  f.dst_voxels = dst->voxels;
  f.dst_tombstones = dst->tombstones;
  VG_RC(refuse(dst, plan_merge(f)));
  if (stats) std::memset(stats, 0, sizeof *stats);
  const size_t upper = (size_t)src->voxels;
  if (upper == 0) {   // an empty source: nothing is launched, nothing changes
    if (stats) stats->seconds = span.seconds();
    return VGICP_OK;
  }
  VG_RC(ensure_table(dst, upper));   // every contributor may open a voxel: the insertion's growth rule, unchanged
  const MergeWork w = merge_work(src->slots, upper);
  VG_RC(ensure_stage(dst, (size_t)w.total));
  if (!dst->h_merge) {
    VG_HIP(dst, dst->h_merge.alloc_mapped(kMergeTotalWords * sizeof(unsigned long long)));
    std::memset(dst->h_merge, 0, kMergeTotalWords * sizeof(unsigned long long));
  }
  if (!src->ev_submap) VG_HIP(dst, src->ev_submap.create(false));
  VG_HIP(dst, hipEventRecord(src->ev_submap, src->stream));
  VG_HIP(dst, hipStreamWaitEvent(dst->stream, src->ev_submap, 0));
  // from here on dst's map changes
  VG_RC(begin_map_update(dst));
  char* work = static_cast<char*>(dst->d_stage.get());
  MergeArgs m;
  std::memset(&m, 0, sizeof m);
  SubmapArgs& a = m.sub;
  a.table = src->table.get();
  a.slots = src->slots;
  a.voxel_size = src->voxel_size;
  for (int e = 0; e < 3; ++e) a.center[e] = params->center[e];
  a.radius = params->radius;
  a.min_count = params->min_count;
  pose_to_state(params->frame, a.pose);
  a.groups = submap_groups(src->slots);
  a.ballots = reinterpret_cast<unsigned long long*>(work + w.submap_at);
  a.group_counts = reinterpret_cast<uint32_t*>(work + w.submap_at + (size_t)a.groups * kSubmapGroupWords * 8);
  a.totals = reinterpret_cast<unsigned long long*>(work + w.submap_at + submap_work_bytes(src->slots) - 4 * 8);
  a.capacity = (uint32_t)upper;
  m.table = dst->table;
  m.mask = (uint32_t)(dst->slots - 1);
  m.n = (uint32_t)upper;
  m.voxel_size = dst->voxel_size;
  m.max_count = params->max_count;
  m.moved = reinterpret_cast<MergeMoved*>(work + w.moved_at);
  m.slot_in = reinterpret_cast<uint32_t*>(work + w.slot_in_at);
  m.slot_out = reinterpret_cast<uint32_t*>(work + w.slot_out_at);
  m.idx_in = reinterpret_cast<uint32_t*>(work + w.idx_in_at);
  m.idx_out = reinterpret_cast<uint32_t*>(work + w.idx_out_at);
  m.split = work + w.split_at;
  m.counters = dst->d_counters;
  m.totals = reinterpret_cast<unsigned long long*>(work + w.totals_at);
  VG_HIP(dst, hipMemsetAsync(m.totals, 0, kMergeTotalWords * sizeof(unsigned long long), dst->stream));
  VG_RC(TimedSpan::begin(dst));
  VG_HIP(dst, launch_map_merge(dst->stream, m, dst->h_merge.dev()));
  VG_RC(TimedSpan::end(dst));
  VG_HIP(dst, hipMemcpyAsync(dst->h_counters, dst->d_counters, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, dst->stream));
  VG_HIP(dst, hipMemcpyAsync(dst->h_merge + 4, m.totals + 4, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, dst->stream));
  VG_HIP(dst, hipStreamSynchronize(dst->stream));   // THE synchronisation; src's work lies in front of dst's
  const unsigned long long* t = dst->h_merge;
  dst->voxels += dst->h_counters[0];
  if (dst->h_counters[1] != 0) return fail(dst, VGICP_ERR_TABLE_FULL, "voxel table probe sequence exhausted");
  if (t[0] > upper) return fail(dst, VGICP_ERR_HIP, "merge: more voxels selected than the source table was known to hold");
  if (stats) {
    stats->selected = t[0];
    stats->too_far = t[1];
    stats->too_few = t[2];
    stats->voxels = t[0] + t[1] + t[2];
    stats->created = dst->h_counters[0];
    stats->updated = t[4];
    stats->frozen = t[5];
    stats->points = t[6];
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    VG_RC(span.device_seconds(dst, &stats->device_seconds));
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}
}  // namespace vgicp_internal
