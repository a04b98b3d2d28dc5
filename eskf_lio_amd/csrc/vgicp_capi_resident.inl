// vgicp_capi_resident.inl — part of vgicp_capi.hip.
// The call frame of the entries over the resident scan at a pose (vgicp_capi_evaluate / _points / _batch / _map_gated
// .inl): what they ask of a context (vgicp_resident_plan.h), the step between their two plans, their timed span and
// the pose view of their launches.  One definition each; the entries keep their layouts, launches and delivery.
namespace {
bool several_devices(const vgicp_ctx* ctx) { return ctx->multi || ctx->owner || ctx->comm || ctx->peers_connected; }
// index of the first of `count` entries that is not finite, or count
size_t first_not_finite(const double* v, size_t count) {
  size_t i = 0;
  while (i < count && std::isfinite(v[i])) ++i;
  return i;
}
ResidentFacts resident_facts(const vgicp_ctx* ctx) {
  return ResidentFacts{several_devices(ctx), ctx->table != nullptr, ctx->scan_ready, /*settled=*/false, ctx->n};
}
int refuse(const vgicp_ctx* ctx, const ResidentVerdict& v) {
  return (v.status == VGICP_OK || !ctx) ? v.status : fail(ctx, v.status, v.text);
}
// Between an entry's two plans: its device current, and what is pending (a scan's kept count, an insertion with it)
// settled, because the capacity checks and the launch geometry are made from n.  *at: the facts as they are then.
int settle_resident(vgicp_ctx* ctx, ResidentFacts* at) {
  VG_HIP(ctx, hipSetDevice(ctx->device));
  VG_RC(settle(ctx));
  *at = resident_facts(ctx);
  at->settled = true;
  return VGICP_OK;
}
// An entry's wall time, from where this is made, and its device time between ev_begin and ev_end (read once the stream
// has been waited for).
struct TimedSpan {
  const double t0 = now_seconds();
  static int begin(vgicp_ctx* ctx) { VG_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream)); return VGICP_OK; }
  static int end(vgicp_ctx* ctx) { VG_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream)); return VGICP_OK; }
  double seconds() const { return now_seconds() - t0; }
  static int device_seconds(vgicp_ctx* ctx, double* out) {
    float ms = 0.f;
    VG_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
    *out = ms * 1e-3;
    return VGICP_OK;
  }
};
// What point_term reads (PointArgs, GateArgs): the settled view, the pose as the kernels take it, the symmetry pair.
PoseView pose_view(const vgicp_ctx* ctx, const double pose16[16]) {
  PoseView v;
  static_cast<ResidentView&>(v) = resident_view(ctx);
  pose_to_state(pose16, v.pose);
  set_symmetry(ctx, &v);
  return v;
}
}  // namespace
