// vgicp_capi_map_gated.inl — part of vgicp_capi.hip.
// The gated insertion of the resident scan (include/vgicp_hip_map_gated.h) behind its entry points in
// libvgicp_hip_map_gated.so: the refusals (plan_insert's for the gated entries, then plan_gate: vgicp_map_plan.h), the
// settling, and the call of insert_points (vgicp_capi_map.inl) with a GateCall — the one place an insertion is launched.
namespace {
GateFacts gate_facts(const vgicp_ctx* ctx, const double* transform, double gate) {
  GateFacts f;
  static_cast<ResidentFacts&>(f) = resident_facts(ctx);
  f.transform_finite = first_not_finite(transform, 16) == 16;
  f.gate = gate;
  return f;
}
// plan_insert's facts: a multi-device context keeps its map and scan in its sub-contexts, so the first of them answers
// "is there a map, is a scan resident" (rule 3 comes before rule 6, which then refuses the context for what it is)
const vgicp_ctx* facts_of(const vgicp_ctx* ctx) { return ctx->multi ? vgicp_multi_api::first(ctx) : ctx; }
}  // namespace

namespace vgicp_internal {
int map_insert_resident_gated(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, double gate,
                              size_t capacity, uint8_t* kept, vgicp_gated_insert_stats* stats) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  const TimedSpan span;
  // as vgicp_map_insert_resident: what is pending is settled before anything is judged (a context of several devices
  // is refused below by what it is, not by what it has pending)
  if (!several_devices(ctx)) VG_RC(settle(ctx));
  const InsertVerdict v = insert_verdict(facts_of(ctx), InsertEntry::ResidentGated, transform != nullptr, max_points_per_voxel, facts_of(ctx)->n);
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  GateFacts facts = gate_facts(ctx, transform, gate);
  facts.kept_given = kept != nullptr;
  facts.capacity = capacity;
  const GateVerdict g = plan_gate(facts);
  if (g.status != VGICP_OK) {
    if (g.rule == 7 && stats) stats->points = ctx->n;
    return fail(ctx, g.status, g.text);
  }
  const size_t n = ctx->n;
  size_t new_voxels = 0;
  const uint64_t launches0 = g_kernel_launches;
  if (!v.nothing_to_do) {
    VG_HIP(ctx, hipSetDevice(ctx->device));
    const GateCall call{gate, kept, /*timed=*/true};
    const int rc = insert_points(ctx, ctx->d_scan_aos, ctx->d_scan_aos + 3 * ctx->scan_capacity, n, transform, max_points_per_voxel,
                                 nullptr, resident_lists_stay_short(ctx), /*deferred=*/false, &new_voxels, &call);
    // the decision's counts came with the insertion's: read whatever the insertion's own verdict is
    const uint32_t* totals = ctx->h_ins_counters + kGateWord;
    uint32_t seen[3];
    for (int k = 0; k < 3; ++k) {
      seen[k] = totals[k] - ctx->gate_seen[k];
      if (rc == VGICP_OK) ctx->gate_seen[k] = totals[k];
    }
    if (rc != VGICP_OK) {
      (void)hipStreamSynchronize(ctx->stream);
      // (the running totals on the device are what they are: the next reader takes the difference from here)
      VG_HIP(ctx, hipMemcpy(ctx->gate_seen, ctx->d_ins_counters + kGateWord, sizeof ctx->gate_seen, hipMemcpyDeviceToHost));
      return rc;
    }
    user_copies_finish(ctx);
    ctx->gated_points += n;
    ctx->gated_refused += seen[1];
    if (stats) {
      stats->matched = seen[0];
      stats->refused = seen[1];
      stats->not_finite = seen[2];
    }
  } else if (stats) {
    stats->matched = stats->refused = stats->not_finite = 0;
  }
  if (stats) {
    stats->points = n;
    stats->new_voxels = new_voxels;
    stats->launches = (int32_t)(g_kernel_launches - launches0);
    stats->reserved = 0;
    stats->device_seconds = 0.0;   // nothing to do: no span was recorded
    if (!v.nothing_to_do) VG_RC(span.device_seconds(ctx, &stats->device_seconds));
    stats->seconds = span.seconds();
  }
  return VGICP_OK;
}

int map_insert_resident_gated_async(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, double gate) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  // as vgicp_map_insert_resident_async: nothing this entry refuses depends on the scan's size
  const InsertVerdict v = insert_verdict(facts_of(ctx), InsertEntry::ResidentGatedAsync, transform != nullptr, max_points_per_voxel, facts_of(ctx)->n);
  if (v.status != VGICP_OK) return fail(ctx, v.status, v.text);
  const GateVerdict g = plan_gate(gate_facts(ctx, transform, gate));
  if (g.status != VGICP_OK) return fail(ctx, g.status, g.text);
  VG_RC(settle_if_pending(ctx));
  if (ctx->n == 0) return VGICP_OK;
  VG_HIP(ctx, hipSetDevice(ctx->device));
  const GateCall call{gate, nullptr, false};
  VG_RC(insert_points(ctx, ctx->d_scan_aos, ctx->d_scan_aos + 3 * ctx->scan_capacity, ctx->n, transform, max_points_per_voxel,
                      nullptr, resident_lists_stay_short(ctx), /*deferred=*/true, nullptr, &call));
  ctx->gated_points += ctx->n;
  return VGICP_OK;
}

int map_gated_totals(vgicp_ctx* ctx, uint64_t* points, uint64_t* refused) {
  if (!ctx) return VGICP_ERR_BAD_ARGUMENT;
  if (!several_devices(ctx)) VG_RC(settle(ctx));
  if (points) *points = ctx->gated_points;
  if (refused) *refused = ctx->gated_refused;
  return VGICP_OK;
}
}  // namespace vgicp_internal
