// vgicp_map_carve.hip — libvgicp_hip_map_carve.so: the entry points of include/vgicp_hip_map_carve.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entries only: the handshake with the module that made the context, then the forward to
// vgicp_internal:: (vgicp_capi_map_carve.inl), inside the module beside the kernels.  Built from the same
// vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

// rules 1 and 2 of the header's list are the handshake; what it leaves for a context of another build
static const char kOtherBuild[] = "context and libvgicp_hip_map_carve.so are not from one build of the module";

extern "C" {

int vgicp_map_carve_resident(vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params* params, size_t capacity,
                             int32_t* removed_keys, size_t* removed, vgicp_carve_stats* stats) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_carve_resident(ctx, transform, params, capacity, removed_keys, removed, stats);
}

int vgicp_map_carve_resident_async(vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params* params) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_carve_resident_async(ctx, transform, params);
}

int vgicp_map_carve_totals(vgicp_ctx* ctx, uint64_t* rays, uint64_t* removed) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_carve_totals(ctx, rays, removed);
}
}  // extern "C"
