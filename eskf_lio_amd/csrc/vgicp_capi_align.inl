// vgicp_capi_align.inl — part of vgicp_capi.hip.
// ICP::align's launch schedule (reference src/Registration.cpp:15-28).  One place each for: the verdict on a persistent
// launch (launch_committed), what a give-up costs (count_fallback), the exchange's rotation (advance_exchange,
// settle_after_launch), the report (report_align); then the two paths of a resident scan, align_persistent and
// align_on_loop (RCCL all-reduce between launches with a communicator), behind run_align, which asks plan_align.
namespace {
// Workgroups of one round's launch over n points at this block size (also the rows per pose of an evaluation).
uint32_t iterate_grid(uint32_t n, uint32_t block) {
  const uint32_t workers = block - 64;  // wave 0 of a workgroup solves, the rest own points
  return std::min<uint32_t>(std::max<uint32_t>((n + workers - 1) / workers, 1), kMaxIterBlocks);
}
uint32_t iterate_grid(const vgicp_ctx* ctx) { return iterate_grid(ctx->n, (uint32_t)ctx->iter_block); }

IterArgs base_args(const vgicp_ctx* ctx) {
  IterArgs a;
  std::memset(&a, 0, sizeof a);
  static_cast<ResidentView&>(a) = resident_view(ctx);
  a.log = ctx->d_log_rows();
  a.stamps = ctx->d_stamps;
  a.memo = static_cast<int4*>(ctx->d_memo.get());
  a.memo_valid = 0;   // the caller knows which launch of the align this is
  set_symmetry(ctx, &a);
  // the dense record copy (tables far beyond the caches' reach): used where it is current — the aligns that reach the
  // loop after a persistent launch has rebuilt it, or run_align's own ensure_dense
  a.dense = (ctx->d_dense && ctx->dense_version == ctx->map_version && ctx->slots >= ctx->dense_slots_threshold &&
             ctx->dense_slots_threshold != 0 && ctx->view_level == 0) ? ctx->d_dense : nullptr;   // a level never uses it
  return a;
}

int load_rccl(vgicp_ctx* ctx) {
  if (ctx->rccl.lib) return VGICP_OK;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* lib = nullptr;
  for (const char* nm : names) {
    lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (lib) break;
  }
  if (!lib) return fail(ctx, VGICP_ERR_RCCL, std::string("cannot load librccl: ") + dlerror());
  RcclApi api;
  api.lib = lib;
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
  api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(lib, "ncclAllReduce"));
  api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(lib, "ncclAllGather"));
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
  if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce)
    return fail(ctx, VGICP_ERR_RCCL, "librccl lacks a required symbol");
  ctx->rccl = api;
  return VGICP_OK;
}

int fail_rccl(const vgicp_ctx* ctx, int code, const char* what) {
  const char* txt = ctx->rccl.GetErrorString ? ctx->rccl.GetErrorString(code) : "?";
  return fail(ctx, VGICP_ERR_RCCL, std::string(what) + ": " + txt);
}

// IterArgs of launch j of an align: state and rows ping-pong, launch 0 writes every point's memo.  The prologue reads
// round j-1's rows: `summed` = the ONE row in d_sums (RCCL's all-reduce, the group's host sum), else the body_grid rows
// launch j-1 wrote.
IterArgs launch_args(const vgicp_ctx* ctx, const IterArgs& base, int j, uint32_t body_grid, bool summed) {
  IterArgs a = base;
  a.state_in = ctx->d_state + (j & 1);
  a.state_out = ctx->d_state + ((j + 1) & 1);
  a.rows = ctx->d_rows[j & 1];
  a.memo_valid = j > 0 ? 1u : 0u;
  a.prev = summed ? ctx->d_sums : ctx->d_rows[(j + 1) & 1];
  a.prev_rows = j > 0 ? (summed ? 1u : body_grid) : 0u;
  return a;
}

// Enqueue launch j of an align on the context's stream.  Launch j's prologue closes round j-1 (fold
// its rows, solve, advance the pose) and its body accumulates round j; the launch after the last
// round is prologue-only and runs as a single workgroup (`closing`).  With a communicator each body
// launch is followed by this rank's row fold and the 256-byte all-reduce the next prologue reads.
int enqueue_launch(vgicp_ctx* ctx, const IterArgs& base, int j, uint32_t body_grid, bool closing, bool use_comm) {
  const IterArgs a = launch_args(ctx, base, j, body_grid, use_comm);
  if (closing) VG_HIP(ctx, launch_close(ctx->stream, a, ctx->iter_block));
  else VG_HIP(ctx, launch_iterate(ctx->stream, a, body_grid, ctx->iter_block));
  if (use_comm && !closing) {
    VG_HIP(ctx, launch_fold_rows(ctx->stream, a.rows, body_grid, a.state_out, ctx->d_sums));
    const int rc = ctx->rccl.AllReduce(ctx->d_sums, ctx->d_sums, kSlots, kNcclDouble, kNcclSum, ctx->comm, ctx->stream);
    if (rc != 0) return fail_rccl(ctx, rc, "ncclAllReduce");
  }
  return VGICP_OK;
}

int check_params(const vgicp_ctx* ctx, const vgicp_params* p) {
  if (!p) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "params is NULL");
  if (p->max_iteration < 0) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "max_iteration < 0");
  return VGICP_OK;
}

void pose_to_state(const double* m16, double* pose12) {
  Pose T;
  pose_from_mat4(m16, T);
  for (int k = 0; k < 9; ++k) pose12[k] = T.R[k];
  for (int k = 0; k < 3; ++k) pose12[9 + k] = T.t[k];
}
void state_to_pose(const double* pose12, double* m16) {
  Pose T;
  for (int k = 0; k < 9; ++k) T.R[k] = pose12[k];
  for (int k = 0; k < 3; ++k) T.t[k] = pose12[9 + k];
  pose_to_mat4(T, m16);
}

// Put the exchange buffers of the persistent launch into their initial state (everything unset, round 0):
// at context creation and after a launch that gave up.
int reset_persistent_exchange(vgicp_ctx* ctx) {
  const size_t rw = persistent_rows_words(), pw = persistent_parts_words();
  unsigned long long* img = static_cast<unsigned long long*>(ctx->h_exchange_image.get());
  persistent_exchange_image(ctx->persist_grid, img, img + rw);
  VG_HIP(ctx, hipMemcpyAsync(ctx->d_rows_persist, img, rw * 8, hipMemcpyHostToDevice, ctx->stream));
  VG_HIP(ctx, hipMemcpyAsync(ctx->d_parts_persist, img + rw, pw * 8, hipMemcpyHostToDevice, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->persist_round0 = 0;
  return VGICP_OK;
}

// A table that is far larger than what caches and TLBs reach (2^24 slots = 2 GiB and more: BASELINE config C5 has
// 8.6 GB) gets a dense copy of its FULL records for the several-points-per-thread launch: tools/micro/gather_pieces
// measured 6.7 ns per random 128-byte line and CU out of a 5-10 GB table against 5.4 ns out of 2.5 GB, and a cliff for
// more lines in flight above 4 GB.  Smaller tables (C2: 512 MB) never use it.  VGICP_DENSE_SLOTS (read when the context is created) overrides the threshold, 0 = never.
bool large_table(const vgicp_ctx* ctx) {
  if (ctx->view_level != 0) return false;   // a stage of vgicp_align_resident_levels: the dense copy is the map's, not a level's
  return ctx->table && ctx->dense_slots_threshold != 0 && ctx->slots >= ctx->dense_slots_threshold && ctx->voxels > 0;
}
bool wants_dense(const vgicp_ctx* ctx, uint32_t n_upper) { return large_table(ctx) && !one_point_per_thread(n_upper, ctx->persist_grid); }
// Storage of the dense copy: sized when the TABLE is (re)allocated (vgicp_map_reset, a growing upsert / insertion) —
// never inside an align.  The table keeps FULL + tombstones + incoming <= slots / 2, so slots / 2 records always suffice.
int reserve_dense(vgicp_ctx* ctx) {
  if (!ctx->table || ctx->dense_slots_threshold == 0 || ctx->slots < ctx->dense_slots_threshold) return VGICP_OK;
  const uint64_t cap = ctx->slots / 2;
  if (cap > ctx->dense_capacity) {
    if (ctx->d_dense) VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->dense_capacity = 0;
    ctx->dense_version = 0;
    VG_HIP(ctx, ctx->d_dense.alloc(cap * sizeof(VoxelRecord)));
    ctx->dense_capacity = cap;
  }
  const uint32_t nb = table_dense_blocks(ctx->slots);
  if (nb + 1 > ctx->dense_counts_capacity) {
    if (ctx->d_dense_counts) VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->dense_counts_capacity = 0;
    VG_HIP(ctx, ctx->d_dense_counts.alloc((size_t)(nb + 1) * sizeof(uint32_t)));
    ctx->dense_counts_capacity = nb + 1;
  }
  return VGICP_OK;
}
// The align's part: rebuild the copy (three launches, no allocation) when the map changed since the last align.
// *usable = false when there is no storage for it (the threshold was lowered after the table was made): the launch then
// simply reads the table.
int ensure_dense(vgicp_ctx* ctx, bool* usable) {
  *usable = false;
  const uint32_t nb = table_dense_blocks(ctx->slots);
  if (!ctx->d_dense || ctx->dense_capacity < ctx->slots / 2 || nb + 1 > ctx->dense_counts_capacity) return VGICP_OK;
  *usable = true;
  if (ctx->dense_version == ctx->map_version) return VGICP_OK;
  VG_HIP(ctx, launch_table_dense(ctx->stream, ctx->table, ctx->slots, ctx->d_dense, ctx->dense_capacity, ctx->d_dense_counts));
  ctx->dense_version = ctx->map_version;
  return VGICP_OK;
}

// ---- one place each: verdict, fallback account, rotation, report ------------------------------------------------------
// Whether a persistent launch's result may be used: the echo of its sequence number is there, workgroup 0's loop ran to
// its end, and NOBODY gave up — `abort_word` is the header's abort_seq for the single and the fused launch, the ONE shared
// word of a team launch.  (Echo and commit WITH the abort word: workgroup 0 arrived late, found every row in place and
// finished while another workgroup had already stopped waiting — its rows of the later rounds are missing.)
bool launch_committed(const AlignState& st, uint32_t seq, uint32_t abort_word) {
  return st.seq == seq && st.outcome == kOutcomeCommitted && abort_word != seq;
}

// What a give-up costs a context that runs alone: counted, the next aligns stay on the loop, one line (the first time, or
// VGICP_VERBOSE).  Not for: a fused launch whose copy threads were slow, a sub-context of a group, the peer verdict.
void count_fallback(vgicp_ctx* ctx, const char* what, const char* also) {
  ++ctx->persistent_fallbacks;
  ctx->persistent_cooldown = kPersistentCooldownAligns;
  if (ctx->persistent_fallbacks == 1 || ctx->dev.verbose)
    std::fprintf(stderr, "[vgicp] %s (fallback #%llu): using one launch per iteration for %sthe next %d aligns\n", what,
                 (unsigned long long)ctx->persistent_fallbacks, also, kPersistentCooldownAligns);
}

// The exchange buffers rotate by round % 3 and the round number runs on from launch to launch: a committed launch's rounds.
void advance_exchange(vgicp_ctx* ctx, const AlignState& st, bool multi) {
  ctx->persist_round0 = (ctx->persist_round0 + (uint32_t)st.iteration) % 3u;
  if (multi) ctx->mail_round0 += (uint32_t)st.iteration;
}

// The frame's ONE synchronisation has happened: what was deferred is known now (a pending scan's size and verdict, the
// counts of the previous frame's map insertion).  When that fails the launch itself may well have completed: the
// exchange's rotation is kept in step before the failure is reported.
int settle_after_launch(vgicp_ctx* ctx, const AlignState& st, uint32_t seq, bool multi) {
  const int rc_scan = settle_scan(ctx);
  const int rc_ins = settle_insert(ctx);
  if (rc_scan == VGICP_OK && rc_ins == VGICP_OK) return VGICP_OK;
  if (launch_committed(st, seq, st.abort_seq)) advance_exchange(ctx, st, multi);
  else (void)reset_persistent_exchange(ctx);
  return rc_scan != VGICP_OK ? rc_scan : rc_ins;
}

// The per-round rows of a log as the caller gets them.
void report_rows(int rounds, const double* log, uint64_t* corr_count, double* normal_eq) {
  for (int it = 0; it < rounds; ++it) {
    const double* row = log + (size_t)it * kSlots;
    if (corr_count) corr_count[it] = (uint64_t)row[kCountSlot];
    if (normal_eq) std::memcpy(normal_eq + (size_t)it * kNormalEq, row, kNormalEq * sizeof(double));
  }
}
int report_pose(const vgicp_ctx* ctx, const AlignState& st, double* out_pose) {
  state_to_pose(st.pose, out_pose);
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(out_pose[i])) return fail(ctx, VGICP_ERR_DEGENERATE, "solved pose is not finite (singular normal equations)");
  return VGICP_OK;
}
// An align's final state and log as out_pose, vgicp_stats and the status.
int report_align(const vgicp_ctx* ctx, const AlignState& st, const double* log, int world, int launches, double device_seconds,
                 double t0, double* out_pose, vgicp_stats* stats) {
  if (stats) {
    stats->iterations = st.iteration;
    stats->converged = st.converged;
    stats->world_size = world;
    stats->launches = launches;
    stats->device_seconds = device_seconds;
    report_rows(st.iteration, log, stats->corr_count, stats->normal_eq);
    stats->seconds = now_seconds() - t0;
  }
  return report_pose(ctx, st, out_pose);
}

// developer aid: where the host time of an align goes (read once per process, by the first align that gets here)
bool trace_align() { static const bool on = std::getenv("VGICP_TRACE_ALIGN") != nullptr; return on; }

// ---- the persistent launch --------------------------------------------------------------------------------------------
// What EVERY persistent launch is told (single, fused, teams): the scan, the table, the thresholds, a sequence number.
void persistent_args_common(vgicp_ctx* ctx, const vgicp_params* params, PersistArgs* out) {
  PersistArgs& a = *out;
  std::memset(&a, 0, sizeof a);
  static_cast<ResidentView&>(a) = resident_view(ctx);   // n of a pending scan: the raw count, an upper bound
  a.seq = ++ctx->persist_seq == 0 ? ++ctx->persist_seq : ctx->persist_seq;  // never 0
  a.cosine_threshold = params->cosine_threshold;
  a.translation_sq_threshold = params->translation_sq_threshold;
  a.max_iteration = params->max_iteration;
}

// The arguments of the single persistent launch, and the header row of the pinned log reset for it: everything the
// host does before the launch (never allocates; the dense copy is rebuilt only when the map changed).
int persistent_args(vgicp_ctx* ctx, const double* guess, const vgicp_params* params, PersistArgs* out) {
  static_assert(sizeof(AlignState) <= kSlots * sizeof(double), "the state must fit the log's header row");
  const uint32_t grid = ctx->persist_grid;  // always the same, all resident: the exchange buffers rely on it
  PersistArgs& a = *out;
  persistent_args_common(ctx, params, &a);
  a.n_dev = ctx->scan_pending ? ctx->d_counters : nullptr;  // a pending scan's kept count is read from the device
  a.asym_dev = symmetry_word(ctx);
  a.scan_seq = ctx->scan_seq;
  if (wants_dense(ctx, ctx->n)) {
    bool usable = false;
    VG_RC(ensure_dense(ctx, &usable));   // a no-op unless the map changed since the last align; never allocates
    if (usable) a.dense = ctx->d_dense;
  }
  a.rows = ctx->d_rows_persist;
  a.parts = ctx->d_parts_persist;
  a.round0 = ctx->persist_round0;
  // final state and per-round log go straight into pinned host memory (posted PCIe writes, 5.4 KB per align):
  // no copy-back to enqueue after the launch
  a.state = reinterpret_cast<AlignState*>(ctx->h_log.dev());
  a.log = ctx->h_log_rows_dev();
  // between GPUs the ranks' host threads reach the launch at slightly different times: a rank waits much longer
  // for a peer (~1 s) than for a workgroup of its own device (~50 ms) before it gives up
  const bool multi = ctx->peers_connected && ctx->peer_world > 1;
  a.spin_limit = multi ? ctx->persist_spin_limit * 20u : ctx->persist_spin_limit;
  pose_to_state(guess, a.pose0);
  persistent_lds_plan(ctx->n, grid, &a.memo_points, &a.stash_points, &a.stash_bytes, ctx->persist_lds_budget);
  if (ctx->dev.no_stash) a.stash_points = a.stash_bytes = 0;
  if (ctx->dev.no_memo) a.memo_points = 0;
  a.prefetch_margin = (a.memo_points == 0 && a.stash_points == 0 && one_point_per_thread(ctx->n, grid)) ? ctx->prefetch_margin : 0.0;
  a.stamps = ctx->d_stamps;
  if (robust_on(ctx)) a.robust = robust_args(ctx);   // launch_persistent then takes the robust instantiation
  if (ctx->prior_on) a.prior = prior_args(ctx);      // ... and the pose prior's
  a.world = multi ? (uint32_t)ctx->peer_world : 1u;
  a.rank = multi ? (uint32_t)ctx->peer_rank : 0u;
  a.mail = ctx->d_mail_table;
  a.mail_round0 = ctx->mail_round0;
  a.mail_seq = multi ? ++ctx->mail_seq : 0u;
  // the launch reports into the header row of the pinned log: who gave up (any workgroup) and workgroup 0's verdict
  AlignState* header = reinterpret_cast<AlignState*>(ctx->h_log.get());
  header->abort_seq = 0;
  header->outcome = kOutcomeNone;
  return fetch_insert_totals(ctx);   // normally carried by the preparation's copy
}

// The whole align in one launch, one synchronisation.  *ran = true: the launch committed and is reported; false with
// VGICP_OK: it gave up, is accounted for, and the caller runs the align on the loop.
int align_persistent(vgicp_ctx* ctx, const double* guess, const vgicp_params* params, const AlignPlan& plan, double t0,
                     double* out_pose, vgicp_stats* stats, bool* ran) {
  *ran = false;
  if (ctx->stage_events) { VG_HIP(ctx, hipEventRecord(ctx->ev_stage[2], ctx->stream)); ctx->ev_stage_set[2] = true; }
  PersistArgs a;
  VG_RC(persistent_args(ctx, guess, params, &a));
  const bool multi = a.world > 1;
  const bool trace = trace_align();
  const double ta0 = trace ? now_seconds() : 0.0;
  VG_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
  VG_HIP(ctx, launch_persistent(ctx->stream, a, ctx->persist_grid));
  VG_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
  if (ctx->stage_events) VG_HIP(ctx, hipEventRecord(ctx->ev_stage[3], ctx->stream));
  const double ta1 = trace ? now_seconds() : 0.0;
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const double ta2 = trace ? now_seconds() : 0.0;
  float ms = 0.f;
  VG_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
  if (trace && ta2 - ta0 > 2e-3)
    std::fprintf(stderr, "[vgicp trace] align: enqueue %.3f ms, hipStreamSynchronize %.3f ms, the launch itself %.3f ms (events)\n",
                 (ta1 - ta0) * 1e3, (ta2 - ta1) * 1e3, (double)ms);
  AlignState* result = &ctx->h_state[0];
  std::memcpy(result, ctx->h_log, sizeof(AlignState));
  ++ctx->persistent_launches;
  VG_RC(settle_after_launch(ctx, *result, a.seq, multi));
  if (launch_committed(*result, a.seq, result->abort_seq)) {
    advance_exchange(ctx, *result, multi);
    if (ctx->stage_events) ctx->ev_stage_set[3] = true;
    *ran = true;
    return report_align(ctx, *result, ctx->h_log_rows(), plan.peer_path ? ctx->peer_world : 1, 1, ms * 1e-3, t0, out_pose, stats);
  }
  // An in-kernel wait timed out (a workgroup was not resident: something else holds CUs of this device; or a peer GPU
  // did not deliver).  Put the exchange back into its initial state, use the per-launch loop for this align and the
  // next few, then try the single launch again.
  const bool wg0_committed = launch_committed(*result, a.seq, 0u);   // workgroup 0's own verdict, whoever else gave up
  if (ctx->owner && multi) {
    // a sub-context of an in-process multi-device context: every sub-context's launch has ended when its thread
    // returns, so the group itself counts and cools down (note_fallback), re-arms all mailboxes and runs this align
    // with the rows added on the host
    ++ctx->persistent_fallbacks;
    if (ctx->dev.verbose)
      std::fprintf(stderr, "[vgicp] rank %d of %d: persistent launch did not commit (echo %s, outcome %u, a workgroup gave up: %s, "
                   "rounds reported %d, %u points)\n", ctx->peer_rank, ctx->peer_world, result->seq == a.seq ? "yes" : "no",
                   result->outcome, result->abort_seq == a.seq ? "yes" : "no", result->iteration, ctx->n);
    const int rc_reset = reset_persistent_exchange(ctx);
    return rc_reset != VGICP_OK ? rc_reset : vgicp_internal::kNeedGroupLoop;
  }
  count_fallback(ctx, multi ? "persistent align launch gave up waiting for a workgroup or a peer GPU"
                            : "persistent align launch gave up waiting for a workgroup", "");
  const int rc = reset_persistent_exchange(ctx);
  if (multi) {
    // Between GPUs the outcome is collective (the verdict words at the end of the launch): every rank leaves the
    // mailboxes for good in the SAME align and re-runs it through the host collective, so the all-reduces pair up.
    // A peer's kernel may still be writing into a mailbox, so they are not touched again.
    ctx->peer_enabled = false;
    const bool agreed = result->outcome == kOutcomeAgreedAbort || (result->outcome == kOutcomeNone && !wg0_committed);
    std::fprintf(stderr, "[vgicp] rank %d: the in-kernel exchange between GPUs gave up (%s); this communicator "
                 "continues with one launch + one RCCL all-reduce per iteration\n", ctx->peer_rank,
                 result->outcome == kOutcomeAgreedAbort ? "a peer reported it" :
                 result->outcome == kOutcomeNoAgreement ? "a peer's verdict never arrived" :
                 wg0_committed ? "a workgroup of this rank, after the verdict was sent" : "this rank timed out");
    if (rc == VGICP_OK && !agreed)
      return fail(ctx, VGICP_ERR_RCCL, "the ranks could not agree on the outcome of this align (a peer's verdict is missing "
                  "or this rank's verdict was sent before one of its workgroups gave up): not re-running it alone");
  }
  return rc;
}

// ---- the launch-per-round loop ----------------------------------------------------------------------------------------
// What every align needs before anything is enqueued for it.
int align_ready(vgicp_ctx* ctx, const vgicp_params* params) {
  if (!ctx->table) return fail(ctx, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (!ctx->scan_ready) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  VG_RC(check_params(ctx, params));
  if (robust_on(ctx) && (ctx->comm != nullptr || ctx->peers_connected || ctx->owner != nullptr))
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the robust round (vgicp_hip_robust.h) is set on this context: it aligns on a "
                "single device only, not with a communicator or connected peers");
  if (ctx->prior_on && (ctx->comm != nullptr || ctx->peers_connected || ctx->owner != nullptr))
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "a pose prior (vgicp_hip_prior.h) is set on this context: it aligns on a "
                "single device only, not with a communicator or connected peers");
  return ensure_log(ctx, params->max_iteration);
}

// The loop's start on one device: the initial AlignState, uploaded.
int upload_initial_state(vgicp_ctx* ctx, const double* guess, const vgicp_params* params) {
  AlignState* h0 = &ctx->h_state[0];
  std::memset(h0, 0, sizeof(AlignState));
  pose_to_state(guess, h0->pose);
  h0->cosine_threshold = params->cosine_threshold;
  h0->translation_sq_threshold = params->translation_sq_threshold;
  h0->max_iteration = params->max_iteration;
  h0->done = (params->max_iteration == 0) ? 1 : 0;
  VG_HIP(ctx, hipMemcpyAsync(ctx->d_state, h0, sizeof(AlignState), hipMemcpyHostToDevice, ctx->stream));
  return VGICP_OK;
}

// max_it bodies + the closing prologue; with VGICP_FLAG_PROFILE an event pair per launch (made once, kept).
int loop_launches(vgicp_ctx* ctx, const vgicp_params* params, int* total_launches) {
  *total_launches = params->max_iteration > 0 ? params->max_iteration + 1 : 0;
  if ((params->flags & VGICP_FLAG_PROFILE) == 0) return VGICP_OK;
  for (size_t k = ctx->ev_prof.size(); k < 2 * (size_t)*total_launches; ++k) {
    ctx->ev_prof.emplace_back();
    VG_HIP(ctx, ctx->ev_prof.back().create());
  }
  return VGICP_OK;
}

// The loop's end on the device that reports (ev_begin was recorded in front of launch 0): final state and log come
// back, one synchronisation, the report.
int report_loop(vgicp_ctx* ctx, const vgicp_params* params, int launched, int world, double t0, double* out_pose,
                vgicp_stats* stats) {
  const int max_it = params->max_iteration;
  VG_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
  AlignState* hf = &ctx->h_state[0];
  VG_HIP(ctx, hipMemcpyAsync(hf, ctx->d_state + (launched & 1), sizeof(AlignState), hipMemcpyDeviceToHost, ctx->stream));
  const bool want_log = stats && (stats->corr_count || stats->normal_eq);
  if (want_log && max_it > 0)
    VG_HIP(ctx, hipMemcpyAsync(ctx->h_log_rows(), ctx->d_log_rows(), (size_t)max_it * kSlots * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  if (stats) VG_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
  if (stats && stats->kernel_ms && (params->flags & VGICP_FLAG_PROFILE) != 0) {
    // one entry per body launch (the closing single-workgroup launch is not a round)
    for (int it = 0; it < std::min(launched, max_it); ++it) {
      float k = 0.f;
      VG_HIP(ctx, hipEventElapsedTime(&k, ctx->ev_prof[2 * it], ctx->ev_prof[2 * it + 1]));
      stats->kernel_ms[it] = k;
    }
  }
  return report_align(ctx, *hf, ctx->h_log_rows(), world, launched, ms * 1e-3, t0, out_pose, stats);
}

// One launch per round for the resident scan, which must be settled (RCCL, VGICP_FLAG_NO_PERSISTENT / _PROFILE, a
// cool-down, a launch that has just given up): touches neither the cool-down nor the counters.
int align_on_loop(vgicp_ctx* ctx, const double* guess, const vgicp_params* params, double* out_pose, vgicp_stats* stats,
                  double t0) {
  VG_RC(align_ready(ctx, params));
  const int max_it = params->max_iteration;
  const bool profile = (params->flags & VGICP_FLAG_PROFILE) != 0;
  const int chunk = profile ? 1 : params->chunk_iterations > 0 ? params->chunk_iterations : kDefaultChunk;
  if (ctx->peers_connected && ctx->peer_world > 1 && ctx->comm == nullptr)
    return fail(ctx, VGICP_ERR_RCCL, "the in-kernel exchange between GPUs is not available for this align (gave up earlier, "
                "profiling or VGICP_FLAG_NO_PERSISTENT) and there is no RCCL communicator to fall back to");
  VG_RC(upload_initial_state(ctx, guess, params));
  // a table far beyond the caches' reach: the loop reads remembered records from the dense copy too (rebuilt here
  // when the map changed since; storage was made with the table, nothing is allocated)
  bool usable = false;
  if (large_table(ctx)) VG_RC(ensure_dense(ctx, &usable));
  IterArgs base = base_args(ctx);
  if (robust_on(ctx)) base.robust = robust_args(ctx);   // launch_iterate then takes the robust instantiation
  if (ctx->prior_on) base.prior = prior_args(ctx);      // ... and launch_iterate / launch_close the pose prior's
  const uint32_t grid = iterate_grid(ctx);
  const bool use_comm = ctx->comm != nullptr;
  int total_launches = 0;
  VG_RC(loop_launches(ctx, params, &total_launches));

  VG_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
  int launched = 0;
  int chunks_enqueued = 0, chunks_checked = 0;
  bool finished = total_launches == 0;
  // Keep up to two chunks in flight: enqueue chunk k+1 before looking at chunk k's status, so the
  // device never idles behind the host; launches enqueued past convergence exit at their first load.
  while (!finished) {
    while (launched < total_launches && chunks_enqueued - chunks_checked < kMaxChunksInFlight) {
      // the first chunk carries one extra launch: launch j closes round j-1
      const int todo = std::min(chunk + (launched == 0 ? 1 : 0), total_launches - launched);
      for (int k = 0; k < todo; ++k) {
        const int j = launched + k;
        if (profile) VG_HIP(ctx, hipEventRecord(ctx->ev_prof[2 * j], ctx->stream));
        VG_RC(enqueue_launch(ctx, base, j, grid, /*closing=*/j == max_it, use_comm));
        if (profile) VG_HIP(ctx, hipEventRecord(ctx->ev_prof[2 * j + 1], ctx->stream));
      }
      launched += todo;
      const int slot = chunks_enqueued % kMaxChunksInFlight;
      VG_HIP(ctx, hipMemcpyAsync(&ctx->h_state[1 + slot], ctx->d_state + (launched & 1), sizeof(AlignState), hipMemcpyDeviceToHost, ctx->stream));
      VG_HIP(ctx, hipEventRecord(ctx->ev_chunk[slot], ctx->stream));
      ++chunks_enqueued;
    }
    const int slot = chunks_checked % kMaxChunksInFlight;
    VG_HIP(ctx, hipEventSynchronize(ctx->ev_chunk[slot]));
    ++chunks_checked;
    if (ctx->h_state[1 + slot].done || (launched >= total_launches && chunks_checked == chunks_enqueued))
      finished = true;
  }
  return report_loop(ctx, params, launched, ctx->world_size, t0, out_pose, stats);
}

// vgicp_align_resident on one context: plan, then the persistent launch or the loop (or both, when the launch gives up).
int run_align(vgicp_ctx* ctx, const double* guess, const vgicp_params* params, double* out_pose, vgicp_stats* stats) {
  const double t0 = now_seconds();
  VG_RC(align_ready(ctx, params));
  const AlignPlan plan = plan_align(align_facts(ctx, params, AlignCall::Resident, ctx->n));
  if (plan.path == AlignPath::GroupLoop) return vgicp_internal::kNeedGroupLoop;  // the group's host-summed loop
  if (plan.path == AlignPath::Loop) {
    // the launch-per-round loop sizes its grid from the scan: a pending scan has to be settled first
    VG_RC(settle(ctx));
    if (!ctx->scan_ready) return fail(ctx, VGICP_ERR_NOT_READY, "no scan resident");
  }
  ctx->persistent_cooldown -= plan.cooldown_drop;
  if (plan.path == AlignPath::Persistent) {
    bool ran = false;
    const int rc = align_persistent(ctx, guess, params, plan, t0, out_pose, stats, &ran);
    if (rc != VGICP_OK || ran) return rc;
  }
  return align_on_loop(ctx, guess, params, out_pose, stats, t0);
}

}  // namespace
