// vgicp_points.hip — libvgicp_hip_points.so: the entry point of include/vgicp_hip_points.h.
// A library of its own because libvgicp_hip.so's exported vgicp_* names are pinned to the lists of the headers before
// this one.  It holds the extern "C" entry only: the handshake with the module that made the context, then the forward
// to vgicp_internal::points_resident (vgicp_capi_points.inl), which lives inside the module beside the kernels.  Built
// from the same vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

extern "C" {

int vgicp_points_resident(vgicp_ctx* ctx, const double pose[16], size_t capacity, double* d2, double* sq_error,
                          double* weight, uint8_t* status, size_t n_quantiles, const double* q,
                          vgicp_point_summary* summary, vgicp_point_stats* stats) {
  // rules 1 and 2 of the header's list; rule 2's words are the ones plan_points keeps for it
  PointsFacts other_build;
  other_build.same_build = false;
  VG_RC(layout_handshake(ctx, plan_points(other_build).text));
  return vgicp_internal::points_resident(ctx, pose, capacity, d2, sq_error, weight, status, n_quantiles, q, summary, stats);
}
}  // extern "C"
