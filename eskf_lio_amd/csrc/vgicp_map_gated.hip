// vgicp_map_gated.hip — libvgicp_hip_map_gated.so: the entry points of include/vgicp_hip_map_gated.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entries only: the handshake with the module that made the context, then the forward to
// vgicp_internal:: (vgicp_capi_map_gated.inl), inside the module beside the kernels.  Built from the same
// vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

// rules 1 and 2 of the header's list are the handshake; what it leaves for a context of another build
static const char kOtherBuild[] = "context and libvgicp_hip_map_gated.so are not from one build of the module";

extern "C" {

int vgicp_map_insert_resident_gated(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, double gate,
                                    size_t capacity, uint8_t* kept, vgicp_gated_insert_stats* stats) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_insert_resident_gated(ctx, transform, max_points_per_voxel, gate, capacity, kept, stats);
}

int vgicp_map_insert_resident_gated_async(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel,
                                          double gate) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_insert_resident_gated_async(ctx, transform, max_points_per_voxel, gate);
}

int vgicp_map_gated_totals(vgicp_ctx* ctx, uint64_t* points, uint64_t* refused) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_gated_totals(ctx, points, refused);
}
}  // extern "C"
