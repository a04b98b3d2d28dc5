// vgicp_map_gated.hip — libvgicp_hip_map_gated.so: the entry points of include/vgicp_hip_map_gated.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entries only: the handshake with the module that made the context, then the forward to
// vgicp_internal:: (vgicp_capi_map_gated.inl), inside the module beside the kernels.  Built from the same
// vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

namespace {
// rules 1 and 2 of the header's list: nothing of the context is read or written unless its layout is this build's (the
// text goes where a failed vgicp_create's goes).  *rc: the status to return when the handshake fails.
bool handshake(const vgicp_ctx* ctx, int* rc) {
  *rc = VGICP_ERR_BAD_ARGUMENT;
  if (ctx && !same_build(ctx)) fail(nullptr, *rc, "context and libvgicp_hip_map_gated.so are not from one build of the module");
  return ctx && same_build(ctx);
}
}  // namespace

extern "C" {

int vgicp_map_insert_resident_gated(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, double gate,
                                    size_t capacity, uint8_t* kept, vgicp_gated_insert_stats* stats) {
  int rc = VGICP_OK;
  if (!handshake(ctx, &rc)) return rc;
  return vgicp_internal::map_insert_resident_gated(ctx, transform, max_points_per_voxel, gate, capacity, kept, stats);
}

int vgicp_map_insert_resident_gated_async(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel,
                                          double gate) {
  int rc = VGICP_OK;
  if (!handshake(ctx, &rc)) return rc;
  return vgicp_internal::map_insert_resident_gated_async(ctx, transform, max_points_per_voxel, gate);
}

int vgicp_map_gated_totals(vgicp_ctx* ctx, uint64_t* points, uint64_t* refused) {
  int rc = VGICP_OK;
  if (!handshake(ctx, &rc)) return rc;
  return vgicp_internal::map_gated_totals(ctx, points, refused);
}
}  // extern "C"
