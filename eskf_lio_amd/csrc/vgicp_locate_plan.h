// vgicp_locate_plan.h — what vgicp_locate_resident (include/vgicp_hip_map_locate.h) decides before it touches the device:
// what it refuses, in the header's order, and the geometry of its score launch.  Pure functions of plain facts (no HIP
// call, no context), so that a CPU program can enumerate them (tests/native/locate_plan.cpp).
#pragma once
#include <cstdint>

#include "../../include/vgicp_hip_map_locate.h"
#include "vgicp_resident_plan.h"

namespace vgicp {

// points of the scan that take part: i % stride == 0
inline uint64_t locate_participants(uint64_t n, uint64_t stride) { return (n + stride - 1) / stride; }
// cells of a window, as a wide integer: three half-widths of 32 give 274 625
inline int64_t locate_cells(const int64_t w[3]) { return (2 * w[0] + 1) * (2 * w[1] + 1) * (2 * w[2] + 1); }

struct LocateFacts {
  bool ctx = true;
  bool pointers = true;        // poses, params and best
  uint64_t k = 1;
  int64_t level = 0;           // the rest of params: readable only when `pointers`
  int64_t window[3] = {0, 0, 0};
  uint64_t stride = 1;
  int requested = 0;           // the context's number of levels
  bool poses_finite = true;    // readable only when rules 1 and 2 pass
  ResidentFacts at;
};
using LocateVerdict = ResidentVerdict;
// a level nobody asked for: locate's words, and the submap's (vgicp_submap_plan.h)
constexpr const char* kLevelNotAskedText = "level is above the number of levels asked for: call vgicp_map_levels_build first";

inline LocateVerdict plan_locate(const LocateFacts& f) {
  if (!f.ctx) return {1, VGICP_ERR_BAD_ARGUMENT};
  if (!f.pointers) return {1, VGICP_ERR_BAD_ARGUMENT, "NULL pointer: poses, params and best are required"};
  if (f.k < 1 || f.k > VGICP_LOCATE_MAX_POSES) return {2, VGICP_ERR_BAD_ARGUMENT, "k must be 1 .. VGICP_LOCATE_MAX_POSES"};
  if (f.level < 0 || f.level > VGICP_LEVELS_MAX) return {2, VGICP_ERR_BAD_ARGUMENT, "level must be 0 .. VGICP_LEVELS_MAX"};
  for (int a = 0; a < 3; ++a)
    if (f.window[a] < 0 || f.window[a] > VGICP_LOCATE_MAX_HALF_WIDTH)
      return {2, VGICP_ERR_BAD_ARGUMENT, "a half-width of the window must be 0 .. VGICP_LOCATE_MAX_HALF_WIDTH"};
  if (locate_cells(f.window) > VGICP_LOCATE_MAX_CELLS)
    return {2, VGICP_ERR_BAD_ARGUMENT, "the window has more than VGICP_LOCATE_MAX_CELLS cells"};
  if (f.stride < 1) return {2, VGICP_ERR_BAD_ARGUMENT, "stride must be >= 1"};
  if (f.level > f.requested) return {3, VGICP_ERR_NOT_READY, kLevelNotAskedText};
  if (!f.poses_finite) return {4, VGICP_ERR_BAD_ARGUMENT, "an entry of a pose is not finite"};
  if (f.at.several_devices)
    return {5, VGICP_ERR_BAD_ARGUMENT, "vgicp_locate_resident is not available on multi-device contexts, communicators "
                                       "and peer-connected contexts: the resident scan of a device is a shard there"};
  LocateVerdict v = plan_ready(f.at, 6);   // a map, a scan, and after settling still a scan: all rule 6 here
  if (v.rule != 0) v.rule = 6;
  return v;
}

// The score launch: a workgroup of kLocateBlock threads takes kLocateChunk points that take part, at one pose.
constexpr uint32_t kLocateBlock = 256;
constexpr uint32_t kLocateChunk = 128;
inline uint32_t locate_chunks(uint64_t participants) { return (uint32_t)((participants + kLocateChunk - 1) / kLocateChunk); }

}  // namespace vgicp
