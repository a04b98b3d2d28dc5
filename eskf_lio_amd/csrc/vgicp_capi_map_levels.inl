// vgicp_capi_map_levels.inl — part of vgicp_capi.hip.
// The map's coarser levels (include/vgicp_hip_map_levels.h) behind their entry points in libvgicp_hip_map_levels.so: the
// refusals (plan_levels, vgicp_levels_plan.h), the settling, the lazy rebuild (ensure_levels, which follows
// ensure_dense: checked by every call that reads a level, a no-op unless the map has changed since) and the align in
// stages, each of which is run_align over a level's view (resident_view, vgicp_context.h).
namespace {
LevelsFacts levels_facts(const vgicp_ctx* ctx, LevelsEntry entry) {
  LevelsFacts f;
  f.entry = entry;
  f.ctx = ctx != nullptr;
  if (ctx) {
    f.requested = ctx->levels_requested;
    // as the carving entries: a multi-device context keeps its map and scan in its sub-contexts; rule 6 refuses it first
    f.at = resident_facts(facts_of(ctx));
    f.at.several_devices = several_devices(ctx);
  }
  return f;
}
int refuse_levels(const vgicp_ctx* ctx, const LevelsFacts& f, const LevelsVerdict& v) {
  if (v.rule == 5) return fail(ctx, v.status, "stage " + std::to_string(f.bad_params_stage) + v.text);
  return refuse(ctx, v);
}

void release_levels(vgicp_ctx* ctx, int keep) {
  for (int l = keep; l < VGICP_LEVELS_MAX; ++l) ctx->level[l] = vgicp_ctx::MapLevel{};
  if (keep == 0) {
    ctx->d_level_counts.reset();
    ctx->h_level_counts.reset();
    ctx->level_counts_pending = false;
  }
}

// Every level asked for is what the rule makes of the map as it is now.  The map must be settled (its voxel count sizes
// the tables).  Enqueues only: two launches per level that is out of date, none when the map has not changed since;
// the levels' voxel counts follow in a copy that wait_level_counts waits for.
int ensure_levels(vgicp_ctx* ctx) {
  int first = 0;   // the levels out of date are first + 1 .. levels_requested (they are built in order, so a suffix)
  while (first < ctx->levels_requested && ctx->level[first].version == ctx->map_version) ++first;
  if (first == ctx->levels_requested) return VGICP_OK;
  if (!ctx->d_level_counts) {
    VG_HIP(ctx, ctx->d_level_counts.alloc(2 * VGICP_LEVELS_MAX * sizeof(uint32_t)));
    VG_HIP(ctx, ctx->h_level_counts.alloc(2 * VGICP_LEVELS_MAX * sizeof(uint32_t)));
    VG_HIP(ctx, hipMemsetAsync(ctx->d_level_counts, 0, 2 * VGICP_LEVELS_MAX * sizeof(uint32_t), ctx->stream));
  }
  const uint64_t want = level_slots(ctx->voxels);
  if (want > kMaxSlots) return fail(ctx, VGICP_ERR_TABLE_FULL, "voxel table would exceed 2^32 slots");
  bool idle = false;   // memory that enqueued work may still read is freed only behind a synchronisation
  VG_HIP(ctx, hipMemsetAsync(ctx->d_level_counts + 2 * first, 0, 2 * (size_t)(ctx->levels_requested - first) * sizeof(uint32_t), ctx->stream));
  for (int l = first; l < ctx->levels_requested; ++l) {
    vgicp_ctx::MapLevel& lv = ctx->level[l];
    lv.version = 0;
    if (!lv.table || lv.slots != want) {
      if (lv.table && !idle) { VG_HIP(ctx, hipStreamSynchronize(ctx->stream)); idle = true; }
      lv.slots = 0;
      const hipError_t e = lv.table.alloc(want * sizeof(VoxelRecord));
      if (e != hipSuccess) return fail(ctx, VGICP_ERR_TABLE_FULL, std::string("hipMalloc(level table): ") + hipGetErrorString(e));
      lv.slots = want;
    }
    // slots are cleared before the claim: all bytes zero is SLOT_EMPTY
    VG_HIP(ctx, hipMemsetAsync(lv.table, 0, lv.slots * sizeof(VoxelRecord), ctx->stream));
    const VoxelRecord* fine = l == 0 ? ctx->table.get() : ctx->level[l - 1].table.get();
    const uint64_t fine_slots = l == 0 ? ctx->slots : ctx->level[l - 1].slots;
    VG_HIP(ctx, launch_level_build(ctx->stream, fine, fine_slots, lv.table, lv.slots, ctx->d_level_counts + 2 * l));
    lv.version = ctx->map_version;
  }
  VG_HIP(ctx, hipMemcpyAsync(ctx->h_level_counts, ctx->d_level_counts, 2 * VGICP_LEVELS_MAX * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  ctx->level_counts_pending = true;
  return VGICP_OK;
}
// The levels' voxel counts on the host (one synchronisation, unless a stage's own has brought them already).
int note_level_counts(vgicp_ctx* ctx) {
  if (!ctx->level_counts_pending) return VGICP_OK;
  ctx->level_counts_pending = false;
  for (int l = 0; l < ctx->levels_requested; ++l) {
    ctx->level[l].voxels = ctx->h_level_counts[2 * l];
    if (ctx->h_level_counts[2 * l + 1] != 0) {
      ctx->level[l].version = 0;
      return fail(ctx, VGICP_ERR_TABLE_FULL, "level table probe sequence exhausted");
    }
  }
  return VGICP_OK;
}
int wait_level_counts(vgicp_ctx* ctx) {
  if (!ctx->level_counts_pending) return VGICP_OK;
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return note_level_counts(ctx);
}
}  // namespace

namespace vgicp_internal {
int map_levels_build(vgicp_ctx* ctx, int levels, vgicp_levels_stats* stats) {
  LevelsFacts f = levels_facts(ctx, LevelsEntry::Build);
  f.levels = levels;
  VG_RC(refuse_levels(ctx, f, plan_levels(f)));
  const TimedSpan span;
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  if (levels < ctx->levels_requested) {
    VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    release_levels(ctx, levels);
  }
  ctx->levels_requested = levels;
  const uint64_t launches0 = g_kernel_launches;
  VG_RC(TimedSpan::begin(ctx));
  VG_RC(ensure_levels(ctx));
  VG_RC(TimedSpan::end(ctx));
  const bool launched = g_kernel_launches != launches0;
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  VG_RC(note_level_counts(ctx));
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->voxels[0] = ctx->voxels;
    stats->slots[0] = ctx->slots;
    for (int l = 0; l < levels; ++l) {
      stats->voxels[l + 1] = ctx->level[l].voxels;
      stats->slots[l + 1] = ctx->level[l].slots;
    }
    stats->levels = levels;
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    if (launched) VG_RC(span.device_seconds(ctx, &stats->device_seconds));   // else: an empty span
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}

int map_level_size(vgicp_ctx* ctx, int level, size_t* voxels, size_t* table_slots, double* voxel_size) {
  LevelsFacts f = levels_facts(ctx, LevelsEntry::Size);
  f.level = level;
  VG_RC(refuse_levels(ctx, f, plan_levels(f)));
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  if (level > 0) {
    VG_RC(ensure_levels(ctx));
    VG_RC(wait_level_counts(ctx));
  }
  if (voxels) *voxels = level == 0 ? ctx->voxels : ctx->level[level - 1].voxels;
  if (table_slots) *table_slots = level == 0 ? ctx->slots : ctx->level[level - 1].slots;
  if (voxel_size) *voxel_size = level_voxel_size(ctx->voxel_size, level);
  return VGICP_OK;
}

int map_level_export(vgicp_ctx* ctx, int level, size_t capacity, int32_t* keys, double* means, double* covs, uint64_t* counts,
                     size_t* written) {
  LevelsFacts f = levels_facts(ctx, LevelsEntry::Export);
  f.level = level;
  f.pointers = written != nullptr;
  f.arrays = keys && means && covs && counts;
  VG_RC(refuse_levels(ctx, f, plan_levels(f)));
  if (level == 0) return vgicp_map_export(ctx, capacity, keys, means, covs, counts, written);
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  VG_RC(ensure_levels(ctx));
  VG_RC(wait_level_counts(ctx));
  const vgicp_ctx::MapLevel& lv = ctx->level[level - 1];
  f.something_to_write = capacity != 0 && lv.voxels != 0;
  VG_RC(refuse_levels(ctx, f, plan_levels(f)));
  *written = 0;
  if (!f.something_to_write) return VGICP_OK;
  // from here on as vgicp_map_export, over the level's table
  const size_t cap = std::min<size_t>(capacity, lv.voxels);
  StageLayout lay;
  const size_t o_keys = lay.take(cap * 3 * sizeof(int32_t)), o_means = lay.take(cap * 3 * sizeof(double));
  const size_t o_covs = lay.take(cap * 9 * sizeof(double)), o_counts = lay.take(cap * sizeof(uint64_t));
  VG_RC(ensure_stage(ctx, lay.total));
  int32_t* d_keys = stage_at<int32_t>(ctx, o_keys);
  double *d_means = stage_at<double>(ctx, o_means), *d_covs = stage_at<double>(ctx, o_covs);
  uint64_t* d_counts = stage_at<uint64_t>(ctx, o_counts);
  VG_HIP(ctx, hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(uint32_t), ctx->stream));
  VG_HIP(ctx, launch_map_export(ctx->stream, lv.table, lv.slots, (uint32_t)cap, d_keys, d_means, d_covs, d_counts, ctx->d_counters));
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

int align_resident_levels(vgicp_ctx* ctx, const double guess[16], size_t stages, const int32_t* levels, const vgicp_params* params,
                          double out_pose[16], vgicp_stats* stats) {
  LevelsFacts f = levels_facts(ctx, LevelsEntry::Align);
  f.pointers = guess && levels && params && out_pose;
  f.stages = stages;
  if (f.pointers && stages >= 1 && stages <= (size_t)VGICP_LEVEL_STAGES_MAX) {   // what rules 1 and 2 ask comes first
    f.stage_level_min = *std::min_element(levels, levels + stages);
    f.stage_level_max = *std::max_element(levels, levels + stages);
    f.guess_finite = first_not_finite(guess, 16) == 16;
    for (size_t i = stages; i-- > 0;)
      if (params[i].max_iteration < 0) f.bad_params_stage = (int64_t)i;
  }
  VG_RC(refuse_levels(ctx, f, plan_levels(f)));
  VG_RC(settle_resident(ctx, &f.at));   // the levels are sized from the map's voxel count
  VG_RC(refuse_levels(ctx, f, plan_levels(f)));
  VG_RC(ensure_levels(ctx));            // enqueued in front of the first stage; its counts ride on that stage's wait
  double pose[16];
  std::memcpy(pose, guess, sizeof pose);
  for (size_t i = 0; i < stages; ++i) {
    double next[16];
    ctx->view_level = levels[i];
    const int rc = run_align(ctx, pose, params + i, next, stats ? stats + i : nullptr);
    ctx->view_level = 0;
    if (rc != VGICP_OK) return rc;
    if (i == 0) VG_RC(note_level_counts(ctx));   // every path of run_align that succeeds has waited for the stream
    std::memcpy(pose, next, sizeof pose);
  }
  std::memcpy(out_pose, pose, sizeof pose);
  return VGICP_OK;
}
}  // namespace vgicp_internal
