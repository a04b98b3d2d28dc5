// vgicp_capi_map_checkpoint.inl — part of vgicp_capi.hip.
// The map checkpoint (include/vgicp_hip_map_checkpoint.h) behind its entry points in libvgicp_hip_map_checkpoint.so: the
// refusals (plan_checkpoint, vgicp_checkpoint_plan.h), the settling, the launches (launch_checkpoint, launch_restore:
// vgicp_mapupdate.hip), the one synchronisation of each call, the blob's way through page-locked memory and, for the
// restore, the check (checkpoint_check) in front of everything and the exchange of the table and the raw log behind it.
namespace {
CheckpointFacts checkpoint_facts(const vgicp_ctx* ctx) {
  CheckpointFacts f;
  f.several_devices = several_devices(ctx);
  f.has_map = ctx->table != nullptr;
  return f;
}
// grow-only; nothing is in flight in the old buffer between calls
int ensure_checkpoint_host(vgicp_ctx* ctx, size_t bytes) {
  if (!ctx->h_checkpoint_totals) {
    VG_HIP(ctx, ctx->h_checkpoint_totals.alloc_mapped(4 * sizeof(unsigned long long)));
    std::memset(ctx->h_checkpoint_totals, 0, 4 * sizeof(unsigned long long));
  }
  if (bytes <= ctx->checkpoint_capacity) return VGICP_OK;
  const size_t cap = std::max<size_t>(bytes + bytes / 4, 1u << 20);
  VG_RC(grow_pinned(ctx, &ctx->h_checkpoint, &ctx->checkpoint_capacity, cap, 0));
  ctx->checkpoint_capacity = cap;
  return VGICP_OK;
}
// the entries of the log that a call has to look at (exact after a settle)
uint32_t raw_entries(const vgicp_ctx* ctx) { return (uint32_t)std::min<uint64_t>(ctx->raw_used_upper, ctx->raw_capacity); }
void fill_checkpoint_stats(vgicp_checkpoint_stats* stats, const CheckpointHeader& h) {
  std::memset(stats, 0, sizeof *stats);
  stats->bytes = h.total_bytes;
  stats->voxels = h.voxels;
  stats->tombstones = h.tombstones;
  stats->raw_points = h.raw_points;
}
}  // namespace

namespace vgicp_internal {
int map_checkpoint_size(vgicp_ctx* ctx, size_t* bytes) {
  VG_RC(refuse(ctx, plan_checkpoint(checkpoint_facts(ctx), false)));
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  VG_RC(raw_refuse_if_broken(ctx));
  uint64_t points = 0;
  if (ctx->raw_on && ctx->voxels > 0) {   // as vgicp_map_points_size counts them
    VG_HIP(ctx, hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(uint32_t), ctx->stream));
    VG_HIP(ctx, launch_raw_offsets(ctx->stream, ctx->table, ctx->slots, nullptr, ctx->d_counters));
    VG_HIP(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    points = ctx->h_counters[0];
  }
  *bytes = (size_t)checkpoint_layout(ctx->voxels, ctx->tombstones, points).total;
  return VGICP_OK;
}

int map_checkpoint(vgicp_ctx* ctx, size_t capacity, void* blob, size_t* written, vgicp_checkpoint_stats* stats) {
  VG_RC(refuse(ctx, plan_checkpoint(checkpoint_facts(ctx), false)));
  const TimedSpan span;
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  VG_RC(raw_refuse_if_broken(ctx));
  const uint64_t launches0 = g_kernel_launches;
  const bool raw = ctx->raw_on;
  const uint64_t F = ctx->voxels, T = ctx->tombstones;
  // the raw points are counted by the launches: until then the log's entries bound them (without the store: none)
  const uint64_t room = raw && F > 0 ? raw_entries(ctx) : 0;
  const char* const too_small = "capacity is below the checkpoint's size";
  *written = (size_t)checkpoint_layout(F, T, 0).total;
  if (!raw && capacity < *written) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, too_small);
  CheckpointHeader h;
  h.voxel_size = ctx->voxel_size;
  h.slots = ctx->slots;
  h.voxels = F;
  h.tombstones = T;
  h.flags = raw ? VGICP_CHECKPOINT_RAW_POINTS : 0u;
  const bool launched = F + T > 0;
  if (launched) {
    const CheckpointLayout upper = checkpoint_layout(F, T, room);
    const CheckpointWork w = checkpoint_work(ctx->slots, F, T, raw, room);
    VG_RC(ensure_stage(ctx, w.total));
    VG_RC(ensure_checkpoint_host(ctx, upper.total));
    char* work = static_cast<char*>(ctx->d_stage.get());
    CheckpointArgs a;
    std::memset(&a, 0, sizeof a);
    a.table = ctx->table;
    a.slots = ctx->slots;
    a.groups = submap_groups(ctx->slots);
    a.ballots = reinterpret_cast<unsigned long long*>(work + w.ballots_at);
    a.word_raw = raw ? reinterpret_cast<uint32_t*>(work + w.word_raw_at) : nullptr;
    a.group_counts = reinterpret_cast<uint32_t*>(work + w.counts_at);
    a.totals = reinterpret_cast<unsigned long long*>(work + w.totals_at);
    a.full_capacity = (uint32_t)F;
    a.tomb_capacity = (uint32_t)T;
    a.full_slots = reinterpret_cast<uint32_t*>(work + w.full_at);
    a.tomb_slots = reinterpret_cast<uint32_t*>(work + w.tomb_at);
    a.records = reinterpret_cast<VoxelRecord*>(work + w.records_at);
    a.offsets = raw ? reinterpret_cast<uint32_t*>(work + w.offsets_at) : nullptr;
    double* d_raw_section = reinterpret_cast<double*>(work + w.raw_at);
    char* out = ctx->h_checkpoint;
    VG_RC(TimedSpan::begin(ctx));
    VG_HIP(ctx, launch_checkpoint(ctx->stream, a, ctx->h_checkpoint_totals.dev()));
    if (room > 0)
      VG_HIP(ctx, launch_checkpoint_raw(ctx->stream, ctx->d_raw, (uint32_t)room, ctx->d_ins_counters + 4, ctx->table, ctx->slots, a.offsets,
                                        (uint32_t)room, d_raw_section));
    // the sections to their places in the page-locked blob; of the raw section as much as could be live
    if (F > 0) VG_HIP(ctx, hipMemcpyAsync(out + upper.full_at, a.full_slots, 4 * F, hipMemcpyDeviceToHost, ctx->stream));
    if (T > 0) VG_HIP(ctx, hipMemcpyAsync(out + upper.tomb_at, a.tomb_slots, 4 * T, hipMemcpyDeviceToHost, ctx->stream));
    if (F > 0) VG_HIP(ctx, hipMemcpyAsync(out + upper.records_at, a.records, kCheckpointRecord * F, hipMemcpyDeviceToHost, ctx->stream));
    if (room > 0) VG_HIP(ctx, hipMemcpyAsync(out + upper.raw_at, d_raw_section, 24 * room, hipMemcpyDeviceToHost, ctx->stream));
    VG_RC(TimedSpan::end(ctx));
    VG_HIP(ctx, hipStreamSynchronize(ctx->stream));   // THE synchronisation
    const unsigned long long* totals = ctx->h_checkpoint_totals;
    if (totals[0] != F || totals[1] != T || (raw && totals[2] > room))
      return fail(ctx, VGICP_ERR_HIP, "checkpoint: the table does not hold the voxels and tombstones the context counts");
    h.raw_points = raw ? totals[2] : 0;
  }
  const CheckpointLayout lay = checkpoint_layout(F, T, h.raw_points);
  h.total_bytes = lay.total;
  *written = (size_t)lay.total;
  if (capacity < lay.total) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, too_small);
  if (launched) {
    char* out = ctx->h_checkpoint;
    if (F & 1) std::memset(out + lay.full_at + 4 * F, 0, 4);   // the pads
    if (T & 1) std::memset(out + lay.tomb_at + 4 * T, 0, 4);
    // one pass over the page-locked payload: into the caller's buffer, summed on the way
    h.checksum = checkpoint_copy_checksum(static_cast<char*>(blob) + kCheckpointHeader, out + kCheckpointHeader, lay.total - kCheckpointHeader);
  }
  checkpoint_write_header(blob, h);
  if (stats) {
    fill_checkpoint_stats(stats, h);
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    if (launched) VG_RC(span.device_seconds(ctx, &stats->device_seconds));
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}

int map_restore(vgicp_ctx* ctx, const void* blob, size_t bytes, vgicp_checkpoint_stats* stats) {
  CheckpointFacts f = checkpoint_facts(ctx);
  VG_RC(refuse(ctx, plan_checkpoint(f, true)));
  const TimedSpan span;   // the check is part of the call's wall time
  CheckpointHeader h;
  const int rule = checkpoint_check(blob, bytes, &h);
  if (rule != 0) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, std::string("vgicp_map_restore: the blob fails the check, ") + checkpoint_rule_text(rule));
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  const uint64_t launches0 = g_kernel_launches;
  const bool raw = (h.flags & VGICP_CHECKPOINT_RAW_POINTS) != 0;
  const uint64_t F = h.voxels, T = h.tombstones, P = h.raw_points;
  const CheckpointLayout lay = checkpoint_layout(F, T, P);
  // everything new is allocated before anything old is let go: a failure up to the exchange leaves the old map in place
  DeviceBuf<VoxelRecord> fresh;
  DeviceBuf<RawPoint> log;
  const uint64_t log_capacity = raw ? restore_raw_capacity(P) : 0;
  hipError_t e = fresh.alloc(h.slots * sizeof(VoxelRecord));
  if (e != hipSuccess) return fail(ctx, VGICP_ERR_TABLE_FULL, std::string("hipMalloc(voxel table): ") + hipGetErrorString(e));
  if (raw) {
    e = log.alloc(log_capacity * sizeof(RawPoint));
    if (e != hipSuccess) return fail(ctx, VGICP_ERR_TABLE_FULL, std::string("hipMalloc(raw-point log): ") + hipGetErrorString(e));
  }
  const RestoreWork w = restore_work(F, T, P);
  VG_RC(ensure_stage(ctx, w.total));
  VG_RC(ensure_checkpoint_host(ctx, bytes));
  StreamIdleOnExit idle{ctx->stream};   // behind the local owners: an early return waits before they free
  char* work = static_cast<char*>(ctx->d_stage.get());
  char* in = ctx->h_checkpoint;
  // the payload into page-locked memory of the context's own (the runtime never sees the caller's pages), then the
  // sections to aligned places on the device
  if (bytes > kCheckpointHeader)
    stage_copy(in + kCheckpointHeader, static_cast<const char*>(blob) + kCheckpointHeader, bytes - kCheckpointHeader);
  RestoreArgs a;
  std::memset(&a, 0, sizeof a);
  a.table = fresh;
  a.slots = h.slots;
  a.full_slots = reinterpret_cast<const uint32_t*>(work + w.full_at);
  a.tomb_slots = reinterpret_cast<const uint32_t*>(work + w.tomb_at);
  a.records = reinterpret_cast<const VoxelRecord*>(work + w.records_at);
  a.voxels = (uint32_t)F;
  a.tombstones = (uint32_t)T;
  a.raw = reinterpret_cast<const double*>(work + w.raw_at);
  a.raw_points = (uint32_t)P;
  a.log = raw ? log.get() : nullptr;
  a.log_capacity = (uint32_t)log_capacity;
  a.ctr = ctx->d_ins_counters + 4;
  a.block_sums = reinterpret_cast<uint32_t*>(work + w.sums_at);
  a.totals = reinterpret_cast<unsigned long long*>(work + w.totals_at);
  VG_RC(TimedSpan::begin(ctx));
  VG_HIP(ctx, launch_table_clear(ctx->stream, fresh, h.slots));
  if (F > 0) VG_HIP(ctx, hipMemcpyAsync(work + w.full_at, in + lay.full_at, 4 * F, hipMemcpyHostToDevice, ctx->stream));
  if (T > 0) VG_HIP(ctx, hipMemcpyAsync(work + w.tomb_at, in + lay.tomb_at, 4 * T, hipMemcpyHostToDevice, ctx->stream));
  if (F > 0) VG_HIP(ctx, hipMemcpyAsync(work + w.records_at, in + lay.records_at, kCheckpointRecord * F, hipMemcpyHostToDevice, ctx->stream));
  if (P > 0) VG_HIP(ctx, hipMemcpyAsync(work + w.raw_at, in + lay.raw_at, 24 * P, hipMemcpyHostToDevice, ctx->stream));
  // the log's words {entries, overflowed, scratch}: the rebuild sets the first.  They are the NEW log's from here on: the
  // old map's log is not read again.  EVERY return between here and the exchange leaves an old store whose words say
  // "empty" beside a stale raw_used_upper: the guard marks it broken, so that it refuses until vgicp_map_reset
  struct OldRawStoreGuard {
    vgicp_ctx* ctx;
    bool armed;
    ~OldRawStoreGuard() { if (armed) ctx->raw_broken = true; }
  } old_store{ctx, raw && ctx->raw_on};
  if (raw) VG_HIP(ctx, hipMemsetAsync(ctx->d_ins_counters + 4, 0, 3 * sizeof(uint32_t), ctx->stream));
  VG_HIP(ctx, launch_restore(ctx->stream, a));
  VG_RC(TimedSpan::end(ctx));
  const hipError_t waited = hipStreamSynchronize(ctx->stream);   // THE synchronisation
  idle.armed = false;
  if (waited != hipSuccess) return fail_hip(ctx, waited, "hipStreamSynchronize(restore)");
  old_store.armed = false;
  // the exchange
  ctx->table = std::move(fresh);
  ctx->slots = h.slots;
  ctx->voxels = F;
  ctx->tombstones = T;
  ctx->voxel_size = h.voxel_size;
  ctx->raw_on = raw;
  ctx->d_raw = std::move(log);   // (without the flag: an empty owner, the old log is freed)
  ctx->raw_capacity = (uint32_t)log_capacity;
  ctx->raw_used_upper = P;
  ctx->raw_broken = false;
  ++ctx->map_version;            // the dense copy and every requested level are out of date
  VG_RC(reserve_dense(ctx));
  if (stats) {
    fill_checkpoint_stats(stats, h);
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    VG_RC(span.device_seconds(ctx, &stats->device_seconds));
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}
}  // namespace vgicp_internal
