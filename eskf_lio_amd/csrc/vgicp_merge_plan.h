// vgicp_merge_plan.h — what vgicp_map_merge (include/vgicp_hip_map_merge.h) decides before it touches the device: what it
// refuses, in the header's order, and the sizes of the scratch its launches work in.  Pure functions of plain facts (no
// HIP call, no context), so that a CPU program can enumerate them (tests/native/merge_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/vgicp_hip_map_merge.h"
#include "vgicp_map_plan.h"
#include "vgicp_submap_plan.h"

namespace vgicp {

struct MergeFacts {
  bool dst = true, src = true, params = true;   // not NULL
  bool dst_build = true, src_build = true;      // made by this build (readable only when not NULL)
  // the rest is readable only when rules 1 and 2 pass
  bool several_devices = false;                 // either context: multi-device, a communicator, peer-connected
  bool same_context = false;                    // dst == src
  bool same_device = true;
  uint64_t reserved = 0;
  bool center_finite = true, frame_finite = true;
  double radius = 0.0;
  bool dst_has_map = true, src_has_map = true;
  uint64_t dst_voxel_bits = 0, src_voxel_bits = 0;   // the two voxel sizes, bit patterns (readable when both have a map)
  bool dst_raw = false;                         // dst keeps raw points
  bool settled = false;                         // both contexts: nothing pending any more
  // once settled
  uint64_t src_voxels = 0;
  uint64_t dst_slots = 0, dst_voxels = 0, dst_tombstones = 0;
};
using MergeVerdict = ResidentVerdict;

// Rules 1 and 2: all that the entry point's own library may ask before the contexts are read
inline MergeVerdict plan_merge_handshake(const MergeFacts& f) {
  if (!f.dst || !f.src || !f.params) return {1, VGICP_ERR_BAD_ARGUMENT, "NULL pointer: dst, src and params are required"};
  if (!f.dst_build || !f.src_build)
    return {2, VGICP_ERR_BAD_ARGUMENT, "context and libvgicp_hip_map_merge.so are not from one build of the module"};
  return {};
}
// the table dst has after the call's growth step: the insertion's rule (ensure_table) for src_voxels incoming voxels
inline TableGrowth plan_merge_growth(const MergeFacts& f) {
  return plan_table_growth(f.dst_has_map, f.dst_slots, f.dst_voxels, f.dst_tombstones, 0, f.src_voxels);
}
inline MergeVerdict plan_merge(const MergeFacts& f) {
  const MergeVerdict first = plan_merge_handshake(f);
  if (first.rule != 0) return first;
  if (f.several_devices)
    return {3, VGICP_ERR_BAD_ARGUMENT, "vgicp_map_merge is not available on multi-device contexts, communicators "
                                       "and peer-connected contexts: the map of a device is a replica there"};
  if (f.same_context) return {4, VGICP_ERR_BAD_ARGUMENT, "dst and src are the same context"};
  if (!f.same_device) return {5, VGICP_ERR_BAD_ARGUMENT, "dst and src are on different devices"};
  if (f.reserved != 0) return {6, VGICP_ERR_BAD_ARGUMENT, "reserved must be 0"};
  if (!f.center_finite || !f.frame_finite) return {7, VGICP_ERR_BAD_ARGUMENT, "an entry of center or frame is not finite"};
  if (!(f.radius >= 0.0)) return {8, VGICP_ERR_BAD_ARGUMENT, "radius must be >= 0 (or +infinity)"};   // a NaN too
  if (!f.dst_has_map || !f.src_has_map) return {9, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first (dst and src)"};
  if (f.dst_voxel_bits != f.src_voxel_bits) return {10, VGICP_ERR_BAD_ARGUMENT, "the voxel sizes of dst and src differ"};
  if (f.dst_raw)
    return {11, VGICP_ERR_BAD_ARGUMENT, "dst keeps raw points (VGICP_OPTION_MAP_RAW_POINTS): a merged voxel has no point list to keep"};
  if (f.settled && f.src_voxels > kScanPointsMax) return {12, VGICP_ERR_BAD_ARGUMENT, "the source holds more voxels than a resident scan may hold"};
  if (f.settled && plan_merge_growth(f).too_large) return {13, VGICP_ERR_BAD_ARGUMENT, "voxel table would exceed 2^32 slots"};
  return {};
}

// ---- the scratch of a call over a source table of `slots` slots that holds `upper` voxels, carved out of the staging
// area: offsets from its (256-byte aligned) base.  A moved contributor is one 128-byte line: a lane of APPLY gathers a
// whole line and nothing else, and the consecutive ranks of MOVE-AND-CLAIM write whole lines ----
struct alignas(128) MergeMoved {
  double mean[3];
  double cov[9];     // column-major
  uint64_t count;
  uint32_t slot;     // of the destination table, or kNoSlot (vgicp_mapupdate.hip): the table was full
  uint32_t pad[5];
};
static_assert(sizeof(MergeMoved) == 128, "one moved contributor = one 128-byte line");
constexpr uint32_t kMergeTotalWords = 8;   // 64-bit: [0..2] SCAN's {selected, too far, too few}, [4] updated, [5] frozen, [6] points
inline uint64_t merge_sort_split_bytes(uint64_t n) { return 2 * (((n / 4 + 64) * 4 + 255) & ~255ull); }   // sortk::split_bytes(n, 4)
struct MergeWork {
  uint64_t submap_at = 0;     // submap_work_bytes(slots): ballots, group counts, SCAN's totals
  uint64_t totals_at = 0;     // kMergeTotalWords
  uint64_t moved_at = 0;      // upper x MergeMoved
  uint64_t slot_in_at = 0, slot_out_at = 0, idx_in_at = 0, idx_out_at = 0;   // upper x 4 each
  uint64_t split_at = 0;      // the sort's splitters
  uint64_t total = 0;
};
inline MergeWork merge_work(uint64_t slots, uint64_t upper) {
  const auto up = [](uint64_t v) { return (v + 255) & ~255ull; };
  const uint64_t m = upper ? upper : 1;
  MergeWork w;
  uint64_t at = 0;
  w.submap_at = at; at += up(submap_work_bytes(slots));
  w.totals_at = at; at += up(kMergeTotalWords * 8);
  w.moved_at = at; at += up(m * sizeof(MergeMoved));
  w.slot_in_at = at; at += up(m * 4);
  w.slot_out_at = at; at += up(m * 4);
  w.idx_in_at = at; at += up(m * 4);
  w.idx_out_at = at; at += up(m * 4);
  w.split_at = at; at += up(merge_sort_split_bytes(m)) + 256;
  w.total = at;
  return w;
}

}  // namespace vgicp
