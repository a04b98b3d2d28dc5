// vgicp_map_merge.hip — libvgicp_hip_map_merge.so: the entry point of include/vgicp_hip_map_merge.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entry only: the handshake with the module that made the contexts — same_build of BOTH, rules 1 and
// 2 of the header's list, decided where the other rules are (plan_merge_handshake, vgicp_merge_plan.h) — then the forward
// to vgicp_internal:: (vgicp_capi_map_merge.inl), inside the module beside the kernels (vgicp_mapupdate.hip).  Built from
// the same vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

namespace {
// the handshake of one of the call's two contexts: there, and stamped by this build
bool from_this_build(const vgicp_ctx* ctx) { return ctx != nullptr && same_build(ctx); }
}  // namespace

extern "C" {

int vgicp_map_merge(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_merge_params* params, vgicp_merge_stats* stats) {
  MergeFacts f;
  f.dst = dst != nullptr;
  f.src = src != nullptr;
  f.params = params != nullptr;
  f.dst_build = from_this_build(dst);
  f.src_build = from_this_build(src);
  const MergeVerdict v = plan_merge_handshake(f);
  // a context of another build is not written to: the text goes where a failed vgicp_create's goes; a NULL pointer's
  // goes into dst only when dst is this build's
  if (v.rule != 0) return vgicp::fail(f.dst_build && v.rule == 1 ? dst : nullptr, v.status, v.text);
  return vgicp_internal::map_merge(dst, src, params, stats);
}
}  // extern "C"
