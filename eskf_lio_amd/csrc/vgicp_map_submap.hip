// vgicp_map_submap.hip — libvgicp_hip_map_submap.so: the entry points of include/vgicp_hip_map_submap.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entries only: the handshake with the module that made the contexts — for the call over two of
// them same_build of BOTH, rules 1 and 2 of the header's list, decided where the other rules are (plan_submap_handshake,
// vgicp_submap_plan.h); for the call over one layout_handshake as every sibling makes it — then the forward
// to vgicp_internal:: (vgicp_capi_map_submap.inl), inside the module beside the kernels (vgicp_mapupdate.hip).  Built from
// the same vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

extern "C" {

int vgicp_scan_from_map(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_submap_params* params, vgicp_submap_stats* stats) {
  SubmapFacts f;
  f.dst = dst != nullptr;
  f.src = src != nullptr;
  f.params = params != nullptr;
  f.dst_build = dst && same_build(dst);
  f.src_build = src && same_build(src);
  const SubmapVerdict v = plan_submap_handshake(f);
  // a context of another build is not written to: the text goes where a failed vgicp_create's goes; a NULL pointer's
  // goes into dst only when dst is this build's
  if (v.rule != 0) return vgicp::fail(f.dst_build && v.rule == 1 ? dst : nullptr, v.status, v.text);
  return vgicp_internal::scan_from_map(dst, src, params, stats);
}

int vgicp_scan_from_map_keys(vgicp_ctx* ctx, size_t capacity, int32_t* keys, uint64_t* counts, size_t* written) {
  VG_RC(layout_handshake(ctx, "context and libvgicp_hip_map_submap.so are not from one build of the module"));
  return vgicp_internal::scan_from_map_keys(ctx, capacity, keys, counts, written);
}
}  // extern "C"
