// vgicp_map_locate.hip — libvgicp_hip_map_locate.so: the entry point of include/vgicp_hip_map_locate.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entry only: the handshake with the module that made the context, then the forward to
// vgicp_internal:: (vgicp_capi_map_locate.inl), inside the module beside the kernels (vgicp_levels.hip).  Built from the
// same vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

extern "C" {

int vgicp_locate_resident(vgicp_ctx* ctx, const double* poses, size_t k, const vgicp_locate_params* params,
                          vgicp_locate_best* best, uint32_t* hits, vgicp_locate_stats* stats) {
  // rule 1 of the header's list
  VG_RC(layout_handshake(ctx, "context and libvgicp_hip_map_locate.so are not from one build of the module"));
  return vgicp_internal::locate_resident(ctx, poses, k, params, best, hits, stats);
}
}  // extern "C"
