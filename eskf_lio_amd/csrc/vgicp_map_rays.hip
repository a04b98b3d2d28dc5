// vgicp_map_rays.hip — libvgicp_hip_map_rays.so: the entry point of include/vgicp_hip_map_rays.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entry only: the handshake with the module that made the context, then the forward to
// vgicp_internal:: (vgicp_capi_map_rays.inl), inside the module beside the kernels.  Built from the same
// vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

extern "C" {

int vgicp_rays_resident(vgicp_ctx* ctx, const double* poses, size_t n_poses, const vgicp_ray_params* params,
                        const vgicp_ray_outputs* per_point, vgicp_ray_counts* counts, vgicp_ray_stats* stats) {
  // rules 1 and 2 of the header's list
  VG_RC(layout_handshake(ctx, "context and libvgicp_hip_map_rays.so are not from one build of the module"));
  return vgicp_internal::rays_resident(ctx, poses, n_poses, params, per_point, counts, stats);
}
}  // extern "C"
