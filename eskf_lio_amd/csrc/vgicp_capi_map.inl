// vgicp_capi_map.inl — part of vgicp_capi.hip.
// The device mirror of LocalMap's voxel grid (reset / upsert / erase / size / export) and LocalMap::updateLocalMap on the
// device (insertion of a scan or of the resident scan, eviction).  What an update refuses and how far the table and the
// raw-point log grow is decided in vgicp_map_plan.h; every insertion is launched by insert_points below.
namespace {
// Every call that changes the map begins its launch here: the call's counter block zeroed, the dense copy out of date.
int begin_map_update(vgicp_ctx* ctx) {
  VG_HIP(ctx, hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(uint32_t), ctx->stream));
  ++ctx->map_version;
  return VGICP_OK;
}
// The tail of a synchronous insertion (launched with d_counters): its counts, and the raw-point log's fill.
int finish_insert(vgicp_ctx* ctx, size_t* new_voxels) {
  VG_HIP(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (ctx->raw_on)
    VG_HIP(ctx, hipMemcpyAsync(ctx->h_raw_ctr, ctx->d_ins_counters + 4, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->voxels += ctx->h_counters[0];
  if (new_voxels) *new_voxels = ctx->h_counters[0];
  if (ctx->h_counters[1] != 0) return fail(ctx, VGICP_ERR_TABLE_FULL, "voxel table probe sequence exhausted");
  return raw_note(ctx, ctx->h_raw_ctr);
}
// The tail of a removal (erase, evict): the voxels it counted are tombstones now.
int finish_removal(vgicp_ctx* ctx, size_t* removed) {
  VG_HIP(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->voxels -= ctx->h_counters[0];
  ctx->tombstones += ctx->h_counters[0];
  if (removed) *removed = ctx->h_counters[0];
  return VGICP_OK;
}

// What plan_insert (vgicp_map_plan.h) decides an insertion entry's refusals by, as this context and this call have them.
// n: the caller's count, or the resident scan's as far as the host knows it.
InsertVerdict insert_verdict(const vgicp_ctx* ctx, InsertEntry entry, bool pointers, size_t max_points_per_voxel, uint64_t n) {
  InsertFacts f;
  f.entry = entry;
  f.has_table = ctx->table != nullptr;
  f.scan_resident = ctx->scan_ready;
  f.pointers = pointers;
  f.points_per_voxel = max_points_per_voxel;
  f.raw_on = ctx->raw_on;
  f.n = n;
  // not several_devices(ctx) (vgicp_capi_resident.inl): what plan_insert refuses is a RANK's shard.  A sub-context of a
  // multi-device context has peers too, but it answers for its group here (facts_of, vgicp_capi_map_gated.inl), which
  // plan_gate then refuses in its own words; the multi-device handle itself never gets here
  f.shard_only = (ctx->comm || ctx->peers_connected) && !ctx->owner;
  return plan_insert(f);
}
bool resident_lists_stay_short(const vgicp_ctx* ctx) {
  return insertion_lists_stay_short(ctx->voxel_size, ctx->prep_voxel, ctx->dev.insert_sort);
}

// LocalMap::updateLocalMap's insertion, the ONE place it is launched from: n > 0 points on this context's device as AoS,
// the entry's verdict passed, its device current.  scratch: map_insert_scratch_bytes(n) the caller carved out of the
// staging area beside its upload, or nullptr: the staging area itself, made large enough here.  deferred: the counts go
// to the running totals behind the counter block and nothing is waited for; settle() (or the next preparation's counter
// copy) reads them.  Else the call returns with the map's new size known.
// gate (the RESIDENT scan only, scratch nullptr): the insertion is a gated one (include/vgicp_hip_map_gated.h).  The
// decision is launched here, behind whatever growth the table needed and in front of the first claim, as a launch of its
// own; its keep plane lies behind the insertion's scratch in the staging area.
struct GateCall {
  double gate;
  uint8_t* kept;            // the caller's array (synchronous entry), or nullptr
  bool timed;               // the entry's TimedSpan begins in front of the decision and ends behind the insertion
};
int insert_points(vgicp_ctx* ctx, const double* d_points, const double* d_covs, size_t n, const double transform[16],
                  size_t max_points_per_voxel, void* scratch, bool short_lists, bool deferred, size_t* new_voxels,
                  const GateCall* gate = nullptr) {
  VG_RC(ensure_table(ctx, n));  // every point may open a voxel (grows / rehashes with a synchronisation when it has to)
  VG_RC(ensure_raw(ctx, n));    // ... and be kept (the log likewise)
  const size_t sb = map_insert_scratch_bytes((uint32_t)n);
  uint8_t* keep = nullptr;
  if (gate) {
    StageLayout lay;
    const size_t o_scratch = lay.take(sb), o_keep = lay.take(n);
    VG_RC(ensure_stage(ctx, lay.total));
    scratch = stage_at<char>(ctx, o_scratch);
    keep = stage_at<uint8_t>(ctx, o_keep);
  } else if (!scratch) {
    VG_RC(ensure_stage(ctx, sb));
    scratch = ctx->d_stage;
  }
  double pose12[12];
  pose_to_state(transform, pose12);
  if (deferred) {
    if (ctx->stage_events) { VG_HIP(ctx, hipEventRecord(ctx->ev_stage[4], ctx->stream)); ctx->ev_stage_set[4] = true; }
    ++ctx->map_version;   // (the running totals are never zeroed: ins_seen remembers what was read)
  } else {
    VG_RC(begin_map_update(ctx));
  }
  if (gate) {
    GateArgs g;
    std::memset(&g, 0, sizeof g);
    static_cast<PoseView&>(g) = pose_view(ctx, transform);   // a gated insertion is the resident scan's: n == ctx->n
    g.gate = gate->gate;
    g.keep = keep;
    g.counters = ctx->d_ins_counters + kGateWord;
    if (gate->timed) VG_RC(TimedSpan::begin(ctx));
    VG_HIP(ctx, launch_gate_decide(ctx->stream, g));
  }
  VG_HIP(ctx, launch_map_insert(ctx->stream, ctx->table, (uint32_t)(ctx->slots - 1), ctx->voxel_size, d_points, d_covs,
                                (uint32_t)n, pose12, (uint64_t)max_points_per_voxel, scratch, sb,
                                deferred ? ctx->d_ins_counters : ctx->d_counters, short_lists, raw_log(ctx), keep));
  if (gate && gate->timed) VG_RC(TimedSpan::end(ctx));
  if (!deferred) {
    // the synchronous gated entry: its counts and the keep plane ride on finish_insert's wait.  The insertion is enqueued
    // by now, so a copy that cannot be enqueued must not keep finish_insert from taking the map's new size: it is
    // reported behind it
    int rc_gate = VGICP_OK;
    if (gate) {
      const hipError_t e = hipMemcpyAsync(ctx->h_ins_counters + kGateWord, ctx->d_ins_counters + kGateWord,
                                          kGateCounters * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
      if (e != hipSuccess) rc_gate = fail_hip(ctx, e, "hipMemcpyAsync(gate counters)");
      arena_reset(ctx);
      if (rc_gate == VGICP_OK && gate->kept) rc_gate = user_d2h(ctx, gate->kept, keep, n);
    }
    const int rc = finish_insert(ctx, new_voxels);
    return rc != VGICP_OK ? rc : rc_gate;
  }
  if (ctx->stage_events) { VG_HIP(ctx, hipEventRecord(ctx->ev_stage[5], ctx->stream)); ctx->ev_stage_set[5] = true; }
  ctx->insert_pending = true;
  ctx->ins_copy_enqueued = false;   // the next preparation's counter copy carries the totals (or settle() fetches them)
  ctx->insert_pending_upper = n;
  if (ctx->raw_on) ctx->raw_used_upper += n;
  ctx->gate_pending = gate != nullptr;
  return VGICP_OK;
}
// what is still pending on the context (a prepared scan's size, an earlier frame's insertion) is settled by one synchronisation
int settle_if_pending(vgicp_ctx* ctx) { return (ctx->scan_pending || ctx->insert_pending) ? settle(ctx) : VGICP_OK; }
}  // namespace

extern "C" {

int vgicp_map_reset(vgicp_ctx* ctx, double voxel_size, size_t capacity_hint) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_reset(ctx, voxel_size, capacity_hint);
  VG_RC(settle(ctx));
  if (!(voxel_size > 0.0) || !std::isfinite(voxel_size))
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "voxel_size must be positive and finite");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->table.reset();
  ctx->slots = ctx->voxels = ctx->tombstones = 0;
  for (auto& l : ctx->level) l = vgicp_ctx::MapLevel{};   // the levels empty with the map; levels_requested stays
  ctx->gated_points = ctx->gated_refused = 0;
  ctx->carve_rays = ctx->carve_removed = 0;
  ++ctx->map_version;
  ctx->voxel_size = voxel_size;
  ctx->raw_hint = capacity_hint;
  const TableGrowth first = plan_first_table(capacity_hint);
  VG_RC(alloc_table(ctx, first, &ctx->table));
  ctx->slots = first.slots;
  if (ctx->raw_on) VG_RC(raw_reset(ctx));   // the store empties with the map
  VG_RC(reserve_dense(ctx));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VGICP_OK;
}

int vgicp_map_upsert(vgicp_ctx* ctx, size_t n, const int32_t* keys, const double* means,
                     const double* covs) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_upsert(ctx, n, keys, means, covs);
  VG_RC(settle(ctx));
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (ctx->raw_on) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the map keeps raw points (VGICP_OPTION_MAP_RAW_POINTS): a mirror batch carries none");
  if (n == 0) return VGICP_OK;
  if (!keys || !means || !covs) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL batch pointer");
  if (n > 0xFFFFFFFFull) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "batch too large");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(ensure_table(ctx, n));
  const size_t kb = n * 3 * sizeof(int32_t), mb = n * 3 * sizeof(double), cb = n * 9 * sizeof(double);
  StageLayout lay;
  const size_t o_keys = lay.take(kb), o_means = lay.take(mb), o_covs = lay.take(cb), o_queue = lay.take(n * sizeof(uint32_t));
  VG_RC(ensure_stage(ctx, lay.total));
  int32_t* d_keys = stage_at<int32_t>(ctx, o_keys);
  double *d_means = stage_at<double>(ctx, o_means), *d_covs = stage_at<double>(ctx, o_covs);
  arena_reset(ctx);
  VG_RC(user_h2d(ctx, d_keys, keys, kb));
  VG_RC(user_h2d(ctx, d_means, means, mb));
  VG_RC(user_h2d(ctx, d_covs, covs, cb));
  VG_RC(begin_map_update(ctx));
  VG_HIP(ctx, launch_upsert(ctx->stream, ctx->table, (uint32_t)(ctx->slots - 1), (uint32_t)n, d_keys, d_means, d_covs,
                            ctx->d_counters, stage_at<uint32_t>(ctx, o_queue)));
  return finish_insert(ctx, nullptr);   // (no raw points here: refused above)
}

int vgicp_map_erase(vgicp_ctx* ctx, size_t n, const int32_t* keys) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_erase(ctx, n, keys);
  VG_RC(settle(ctx));
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (n == 0) return VGICP_OK;
  if (!keys) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL batch pointer");
  if (n > 0xFFFFFFFFull) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "batch too large");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  const size_t kb = n * 3 * sizeof(int32_t);
  VG_RC(ensure_stage(ctx, kb));
  arena_reset(ctx);
  VG_RC(user_h2d(ctx, ctx->d_stage, keys, kb));
  VG_RC(begin_map_update(ctx));
  VG_HIP(ctx, launch_erase(ctx->stream, ctx->table, (uint32_t)(ctx->slots - 1), (uint32_t)n,
                           static_cast<const int32_t*>(ctx->d_stage.get()), ctx->d_counters));
  return finish_removal(ctx, nullptr);
}

int vgicp_map_size(const vgicp_ctx* ctx, size_t* voxels, size_t* table_slots) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_size(ctx, voxels, table_slots);
  VG_RC(settle(const_cast<vgicp_ctx*>(ctx)));  // a deferred insertion
  if (voxels) *voxels = ctx->voxels;
  if (table_slots) *table_slots = ctx->slots;
  return VGICP_OK;
}

int vgicp_map_insert_scan(vgicp_ctx* ctx, size_t n, const double* points, const double* covs,
                          const double transform[16], size_t max_points_per_voxel, size_t* new_voxels) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_insert_scan(ctx, n, points, covs, transform, max_points_per_voxel, new_voxels);
  if (new_voxels) *new_voxels = 0;
  VG_RC(settle(ctx));
  const InsertVerdict v = insert_verdict(ctx, InsertEntry::Scan, points && covs && transform, max_points_per_voxel, n);
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  if (v.nothing_to_do) return VGICP_OK;
  VG_HIP(ctx, hipSetDevice(ctx->device));
  // the scan and the insertion's scratch side by side in the staging area
  StageLayout lay;
  const size_t o_pts = lay.take(n * 3 * sizeof(double)), o_covs = lay.take(n * 9 * sizeof(double));
  const size_t o_scratch = lay.take(map_insert_scratch_bytes((uint32_t)n));
  VG_RC(ensure_stage(ctx, lay.total));
  double *d_pts = stage_at<double>(ctx, o_pts), *d_covs = stage_at<double>(ctx, o_covs);
  arena_reset(ctx);
  VG_RC(user_h2d(ctx, d_pts, points, n * 3 * sizeof(double)));
  VG_RC(user_h2d(ctx, d_covs, covs, n * 9 * sizeof(double)));
  const int rc = insert_points(ctx, d_pts, d_covs, n, transform, max_points_per_voxel, stage_at<char>(ctx, o_scratch),
                               /*short_lists=*/false, /*deferred=*/false, new_voxels);
  // refused on the way (a table that cannot grow): the copies out of the caller's buffers are enqueued already
  if (rc != VGICP_OK) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

int vgicp_map_insert_resident(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel,
                              size_t* new_voxels) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_insert_resident(ctx, transform, max_points_per_voxel, new_voxels, false);
  if (new_voxels) *new_voxels = 0;
  VG_RC(settle(ctx));
  const InsertVerdict v = insert_verdict(ctx, InsertEntry::Resident, transform != nullptr, max_points_per_voxel, ctx->n);
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  if (v.nothing_to_do) return VGICP_OK;
  VG_HIP(ctx, hipSetDevice(ctx->device));
  return insert_points(ctx, ctx->d_scan_aos, ctx->d_scan_aos + 3 * ctx->scan_capacity, ctx->n, transform, max_points_per_voxel,
                       nullptr, resident_lists_stay_short(ctx), /*deferred=*/false, new_voxels);
}

int vgicp_map_insert_resident_async(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_insert_resident(ctx, transform, max_points_per_voxel, nullptr, true);
  // nothing this entry refuses depends on the scan's size; it has to be known only from here on (the align that
  // registered the scan has settled it), and an insertion still pending from an earlier frame is settled by the same
  // synchronisation
  const InsertVerdict v = insert_verdict(ctx, InsertEntry::ResidentAsync, transform != nullptr, max_points_per_voxel, ctx->n);
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  VG_RC(settle_if_pending(ctx));
  if (ctx->n == 0) return VGICP_OK;
  VG_HIP(ctx, hipSetDevice(ctx->device));
  return insert_points(ctx, ctx->d_scan_aos, ctx->d_scan_aos + 3 * ctx->scan_capacity, ctx->n, transform, max_points_per_voxel,
                       nullptr, resident_lists_stay_short(ctx), /*deferred=*/true, nullptr);
}

int vgicp_map_evict(vgicp_ctx* ctx, const double position[3], double distance_threshold, size_t* removed) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_evict(ctx, position, distance_threshold, removed);
  if (removed) *removed = 0;
  VG_RC(settle(ctx));
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (!position) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(begin_map_update(ctx));
  VG_HIP(ctx, launch_map_evict(ctx->stream, ctx->table, ctx->slots, ctx->voxel_size, position,
                               distance_threshold, ctx->d_counters));
  return finish_removal(ctx, removed);
}

int vgicp_map_export(vgicp_ctx* ctx, size_t capacity, int32_t* keys, double* means, double* covs,
                     uint64_t* counts, size_t* written) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return vgicp_multi_api::map_export(ctx, capacity, keys, means, covs, counts, written);
  if (!written) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "written is NULL");
  *written = 0;
  VG_RC(settle(ctx));
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (capacity == 0 || ctx->voxels == 0) return VGICP_OK;
  if (!keys || !means || !covs || !counts) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL array pointer");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cap = std::min<size_t>(capacity, ctx->voxels);
  StageLayout lay;
  const size_t o_keys = lay.take(cap * 3 * sizeof(int32_t)), o_means = lay.take(cap * 3 * sizeof(double));
  const size_t o_covs = lay.take(cap * 9 * sizeof(double)), o_counts = lay.take(cap * sizeof(uint64_t));
  VG_RC(ensure_stage(ctx, lay.total));
  int32_t* d_keys = stage_at<int32_t>(ctx, o_keys);
  double *d_means = stage_at<double>(ctx, o_means), *d_covs = stage_at<double>(ctx, o_covs);
  uint64_t* d_counts = stage_at<uint64_t>(ctx, o_counts);
  VG_HIP(ctx, hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(uint32_t), ctx->stream));
  VG_HIP(ctx, launch_map_export(ctx->stream, ctx->table, ctx->slots, (uint32_t)cap, d_keys, d_means, d_covs, d_counts, ctx->d_counters));
  arena_reset(ctx);
  VG_RC(user_d2h(ctx, keys, d_keys, cap * 3 * sizeof(int32_t)));
  VG_RC(user_d2h(ctx, means, d_means, cap * 3 * sizeof(double)));
  VG_RC(user_d2h(ctx, covs, d_covs, cap * 9 * sizeof(double)));
  VG_RC(user_d2h(ctx, counts, d_counts, cap * sizeof(uint64_t)));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  user_copies_finish(ctx);
  *written = cap;
  return VGICP_OK;
}

// ---- the raw points of the map (include/vgicp_hip_map_points.h) ----
int vgicp_map_points_size(const vgicp_ctx* ctx, size_t* points, size_t* capacity) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return forward_to_first(ctx, [&](vgicp_ctx* lead) { return vgicp_map_points_size(lead, points, capacity); });
  vgicp_ctx* c = const_cast<vgicp_ctx*>(ctx);
  VG_RC(settle(c));
  if (!c->raw_on) return fail(c, VGICP_ERR_NOT_READY, "the map keeps no raw points: set VGICP_OPTION_MAP_RAW_POINTS");
  VG_RC(raw_refuse_if_broken(c));
  size_t total = 0;
  if (c->table && c->voxels > 0) {
    VG_HIP(c, hipSetDevice(c->device));
    VG_HIP(c, hipMemsetAsync(c->d_counters, 0, 4 * sizeof(uint32_t), c->stream));
    VG_HIP(c, launch_raw_offsets(c->stream, c->table, c->slots, nullptr, c->d_counters));
    VG_HIP(c, hipMemcpyAsync(c->h_counters, c->d_counters, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    VG_HIP(c, hipStreamSynchronize(c->stream));
    total = c->h_counters[0];
  }
  if (points) *points = total;
  if (capacity) *capacity = c->raw_capacity;
  return VGICP_OK;
}

int vgicp_map_points_export(vgicp_ctx* ctx, size_t capacity, int32_t* keys, double* points, size_t* written) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (ctx->multi) return forward_to_first(ctx, [&](vgicp_ctx* lead) { return vgicp_map_points_export(lead, capacity, keys, points, written); });
  if (!written) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "written is NULL");
  *written = 0;
  VG_RC(settle(ctx));
  if (!ctx->raw_on) return fail(ctx, VGICP_ERR_NOT_READY, "the map keeps no raw points: set VGICP_OPTION_MAP_RAW_POINTS");
  VG_RC(raw_refuse_if_broken(ctx));
  if (!ctx->table || capacity == 0 || ctx->voxels == 0 || ctx->raw_used_upper == 0) return VGICP_OK;
  if (!keys || !points) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "NULL array pointer");
  VG_HIP(ctx, hipSetDevice(ctx->device));
  // the live points are at most the entries appended (exact after the settle): room for that many, or for capacity
  const uint32_t used = (uint32_t)std::min<uint64_t>(ctx->raw_used_upper, ctx->raw_capacity);
  const size_t room = std::min<size_t>(capacity, used);
  StageLayout lay;
  const size_t o_offsets = lay.take(ctx->slots * sizeof(uint32_t)), o_keys = lay.take(room * 3 * sizeof(int32_t));
  const size_t o_pts = lay.take(room * 3 * sizeof(double));
  VG_RC(ensure_stage(ctx, lay.total));
  uint32_t* offsets = stage_at<uint32_t>(ctx, o_offsets);
  int32_t* d_keys = stage_at<int32_t>(ctx, o_keys);
  double* d_pts = stage_at<double>(ctx, o_pts);
  // 1. every voxel's place in the output (its count points from there) and the total
  VG_HIP(ctx, hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(uint32_t), ctx->stream));
  VG_HIP(ctx, launch_raw_offsets(ctx->stream, ctx->table, ctx->slots, offsets, ctx->d_counters));
  VG_HIP(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t cap = std::min<size_t>(room, ctx->h_counters[0]);
  if (cap == 0) return VGICP_OK;
  // 2. every live entry to its voxel's place + ordinal
  VG_HIP(ctx, launch_raw_scatter(ctx->stream, ctx->d_raw, used, ctx->d_ins_counters + 4, ctx->table, ctx->slots, offsets, (uint32_t)cap,
                                 d_keys, d_pts));
  arena_reset(ctx);
  VG_RC(user_d2h(ctx, keys, d_keys, cap * 3 * sizeof(int32_t)));
  VG_RC(user_d2h(ctx, points, d_pts, cap * 3 * sizeof(double)));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  user_copies_finish(ctx);
  *written = cap;
  return VGICP_OK;
}
}  // extern "C"
