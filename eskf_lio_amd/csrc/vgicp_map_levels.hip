// vgicp_map_levels.hip — libvgicp_hip_map_levels.so: the entry points of include/vgicp_hip_map_levels.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entries only: the handshake with the module that made the context, then the forward to
// vgicp_internal:: (vgicp_capi_map_levels.inl), inside the module beside the kernels (vgicp_levels.hip).  Built from the
// same vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

// rule 1 of the header's list is the handshake; what it leaves for a context of another build
static const char kOtherBuild[] = "context and libvgicp_hip_map_levels.so are not from one build of the module";

extern "C" {

int vgicp_map_levels_build(vgicp_ctx* ctx, int levels, vgicp_levels_stats* stats) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_levels_build(ctx, levels, stats);
}

int vgicp_map_level_size(vgicp_ctx* ctx, int level, size_t* voxels, size_t* table_slots, double* voxel_size) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_level_size(ctx, level, voxels, table_slots, voxel_size);
}

int vgicp_map_level_export(vgicp_ctx* ctx, int level, size_t capacity, int32_t* keys, double* means, double* covs,
                           uint64_t* counts, size_t* written) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::map_level_export(ctx, level, capacity, keys, means, covs, counts, written);
}

int vgicp_align_resident_levels(vgicp_ctx* ctx, const double guess[16], size_t stages, const int32_t* levels,
                                const vgicp_params* params, double out_pose[16], vgicp_stats* stats) {
  VG_RC(layout_handshake(ctx, kOtherBuild));
  return vgicp_internal::align_resident_levels(ctx, guess, stages, levels, params, out_pose, stats);
}
}  // extern "C"
