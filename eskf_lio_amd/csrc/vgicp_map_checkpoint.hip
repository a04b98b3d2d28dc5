// vgicp_map_checkpoint.hip — libvgicp_hip_map_checkpoint.so: the entry points of include/vgicp_hip_map_checkpoint.h.
// A library of its own for the reason vgicp_points.hip gives: libvgicp_hip.so's exported vgicp_* names are pinned.  It
// holds the extern "C" entries only: rules 1 and 2 of the header's lists — the NULL pointers and the handshake with the
// module that made the context, decided where the other rules are (plan_checkpoint_handshake, vgicp_checkpoint_plan.h) —
// then the forward to vgicp_internal:: (vgicp_capi_map_checkpoint.inl), inside the module beside the kernels
// (vgicp_mapupdate.hip).  vgicp_map_checkpoint_info needs no context: it is the plan header's check and nothing else.
// Built from the same vgicp_context.h as the module (one Makefile, one rule set) and linked against it.
#include "vgicp_context.h"

namespace {
// a context of another build is not written to: the text goes where a failed vgicp_create's goes; a NULL pointer's goes
// into ctx only when ctx is this build's
int refuse_entry(vgicp_ctx* ctx, bool pointers) {
  CheckpointFacts f;
  f.pointers = ctx != nullptr && pointers;
  f.same_build = ctx && same_build(ctx);
  const CheckpointVerdict v = plan_checkpoint_handshake(f);
  if (v.rule == 0) return VGICP_OK;
  return vgicp::fail(ctx && same_build(ctx) ? ctx : nullptr, v.status, v.text);
}
}  // namespace

extern "C" {

int vgicp_map_checkpoint_size(vgicp_ctx* ctx, size_t* bytes) {
  VG_RC(refuse_entry(ctx, bytes != nullptr));
  return vgicp_internal::map_checkpoint_size(ctx, bytes);
}

int vgicp_map_checkpoint(vgicp_ctx* ctx, size_t capacity, void* blob, size_t* written, vgicp_checkpoint_stats* stats) {
  VG_RC(refuse_entry(ctx, blob != nullptr && written != nullptr));
  return vgicp_internal::map_checkpoint(ctx, capacity, blob, written, stats);
}

int vgicp_map_checkpoint_info(const void* blob, size_t bytes, vgicp_checkpoint_info* info) {
  if (!blob || !info) return vgicp::fail(nullptr, VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  std::memset(info, 0, sizeof *info);
  CheckpointHeader h;
  std::memset(&h, 0, sizeof h);
  const int rule = checkpoint_check(blob, bytes, &h);
  info->format = h.format;
  info->header_bytes = h.header_bytes;
  info->total_bytes = h.total_bytes;
  info->voxel_size = h.voxel_size;
  info->slots = h.slots;
  info->voxels = h.voxels;
  info->tombstones = h.tombstones;
  info->raw_points = h.raw_points;
  info->flags = h.flags;
  info->record_bytes = h.record_bytes;
  info->checksum = h.checksum;
  info->rule = rule;
  if (rule != 0) return vgicp::fail(nullptr, VGICP_ERR_BAD_ARGUMENT, std::string("the blob fails the check, ") + checkpoint_rule_text(rule));
  return VGICP_OK;
}

int vgicp_map_restore(vgicp_ctx* ctx, const void* blob, size_t bytes, vgicp_checkpoint_stats* stats) {
  VG_RC(refuse_entry(ctx, blob != nullptr));
  return vgicp_internal::map_restore(ctx, blob, bytes, stats);
}
}  // extern "C"
