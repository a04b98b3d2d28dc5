// vgicp_submap_plan.h — what vgicp_scan_from_map (include/vgicp_hip_map_submap.h) decides before it touches the device:
// what it refuses, in the header's order, and the geometry of its three launches.  Pure functions of plain facts (no HIP
// call, no context), so that a CPU program can enumerate them (tests/native/submap_plan.cpp).
#pragma once
#include <cstdint>

#include "../../include/vgicp_hip_map_submap.h"
#include "vgicp_locate_plan.h"

namespace vgicp {

struct SubmapFacts {
  bool dst = true, src = true, params = true;   // not NULL
  bool dst_build = true, src_build = true;      // made by this build (readable only when not NULL)
  // the rest is readable only when rules 1 and 2 pass
  bool several_devices = false;                 // either context: multi-device, a communicator, peer-connected
  bool same_device = true;
  int64_t reserved = 0, level = 0;
  int requested = 0;                            // src's number of levels
  bool center_finite = true, frame_finite = true;
  double radius = 0.0;
  bool src_has_map = true;
  bool settled = false;                         // both contexts: nothing pending any more
  uint64_t voxels = 0;                          // of the source table (an upper bound while a level's count is on its way); once settled
};
using SubmapVerdict = ResidentVerdict;
constexpr uint64_t kScanPointsMax = 0xFFFFFFFFull;   // what vgicp_scan_upload lets through

// Rules 1 and 2: all that the entry point's own library may ask before the contexts are read
inline SubmapVerdict plan_submap_handshake(const SubmapFacts& f) {
  if (!f.dst || !f.src || !f.params) return {1, VGICP_ERR_BAD_ARGUMENT, "NULL pointer: dst, src and params are required"};
  if (!f.dst_build || !f.src_build)
    return {2, VGICP_ERR_BAD_ARGUMENT, "context and libvgicp_hip_map_submap.so are not from one build of the module"};
  return {};
}
inline SubmapVerdict plan_submap(const SubmapFacts& f) {
  const SubmapVerdict first = plan_submap_handshake(f);
  if (first.rule != 0) return first;
  if (f.several_devices)
    return {3, VGICP_ERR_BAD_ARGUMENT, "vgicp_scan_from_map is not available on multi-device contexts, communicators "
                                       "and peer-connected contexts: the resident scan of a device is a shard there"};
  if (!f.same_device) return {4, VGICP_ERR_BAD_ARGUMENT, "dst and src are on different devices"};
  if (f.reserved != 0) return {5, VGICP_ERR_BAD_ARGUMENT, "reserved must be 0"};
  if (f.level < 0 || f.level > VGICP_LEVELS_MAX) return {6, VGICP_ERR_BAD_ARGUMENT, "level must be 0 .. VGICP_LEVELS_MAX"};
  if (f.level > f.requested) return {7, VGICP_ERR_NOT_READY, kLevelNotAskedText};
  if (!f.center_finite || !f.frame_finite) return {8, VGICP_ERR_BAD_ARGUMENT, "an entry of center or frame is not finite"};
  if (!(f.radius >= 0.0)) return {9, VGICP_ERR_BAD_ARGUMENT, "radius must be >= 0 (or +infinity)"};   // a NaN too
  if (!f.src_has_map) return {10, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first"};
  if (f.settled && f.voxels > kScanPointsMax) return {11, VGICP_ERR_BAD_ARGUMENT, "scan too large"};
  return {};
}

// The launches: a workgroup of kSubmapBlock threads takes kSubmapGroupSlots consecutive slots, kSubmapPer per thread; a
// wave's 64 slots of one turn are consecutive, so a group has kSubmapGroupWords ballots, in slot order.
constexpr uint32_t kSubmapBlock = 256, kSubmapPer = 4;
constexpr uint32_t kSubmapGroupSlots = kSubmapBlock * kSubmapPer, kSubmapGroupWords = kSubmapGroupSlots / 64;
inline uint32_t submap_groups(uint64_t slots) { return (uint32_t)((slots + kSubmapGroupSlots - 1) / kSubmapGroupSlots); }
// the call's scratch: the ballots, then the groups' three counts (selected, too far, too few), then the three totals
inline uint64_t submap_work_bytes(uint64_t slots) {
  const uint64_t g = submap_groups(slots);
  return g * kSubmapGroupWords * 8 + ((3 * g * 4 + 7) & ~7ull) + 4 * 8;
}

}  // namespace vgicp
