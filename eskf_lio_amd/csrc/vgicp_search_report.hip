// vgicp_search_report.hip — libvgicp_hip_search_report.so: the entry point of include/vgicp_hip_search_report.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entry only: the handshake with the module that made the context, then the forward to
// vgicp_internal:: (vgicp_capi_prepare.inl), inside the module beside the kernel that counts.  Built from the same
// vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

extern "C" {

int vgicp_prepare_search_report(vgicp_ctx* ctx, vgicp_search_report* report) {
  VG_RC(layout_handshake(ctx, "context and libvgicp_hip_search_report.so are not from one build of the module"));
  return vgicp_internal::prepare_search_report(ctx, report);
}
}  // extern "C"
