// vgicp_levels_plan.h — what the map levels (include/vgicp_hip_map_levels.h) decide before they touch the device: how
// large a level's table is made, and what each of the four entry points refuses, in the header's order.  Pure functions
// of plain facts (no HIP call, no context), so that a CPU program can enumerate them (tests/native/levels_plan.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/vgicp_hip_map_levels.h"
#include "vgicp_map_plan.h"
#include "vgicp_resident_plan.h"

namespace vgicp {

// A level has at most as many voxels as the level below it, and so at most as many as the map: with two slots per voxel
// of the map (a count the host holds once it has settled; no round trip between levels) at least half of the slots of
// every level stay EMPTY, which is what find_voxel's walk relies on.
inline uint64_t level_slots(uint64_t map_voxels) { return next_pow2(std::max<uint64_t>(kMinSlots, map_voxels * 2)); }
// the voxel size of level l: exact, a power of two times the map's
inline double level_voxel_size(double voxel_size, int level) { return std::ldexp(voxel_size, level); }

enum class LevelsEntry { Build, Size, Export, Align };
struct LevelsFacts {
  LevelsEntry entry = LevelsEntry::Build;
  bool ctx = true;
  bool pointers = true;           // Export: written; Align: guess, levels, params, out_pose.  Build, Size: none is asked
  int64_t levels = 0;             // Build: the count asked for
  int64_t level = 0;              // Size, Export
  uint64_t stages = 1;            // Align
  int64_t stage_level_min = 0, stage_level_max = 0;   // Align: over the stages (readable only when rules 1 and 2 of `stages` pass)
  int requested = 0;              // the context's number of levels
  bool guess_finite = true;       // Align
  int64_t bad_params_stage = -1;  // Align: the first stage whose max_iteration < 0, or -1
  bool arrays = true;             // Export: keys, means, covs and counts are all there
  bool something_to_write = false;   // Export, once the level is built: capacity > 0 and the level holds a voxel
  ResidentFacts at;
};
using LevelsVerdict = ResidentVerdict;

inline LevelsVerdict plan_levels(const LevelsFacts& f) {
  const bool align = f.entry == LevelsEntry::Align, build = f.entry == LevelsEntry::Build;
  if (!f.ctx) return {1, VGICP_ERR_BAD_ARGUMENT};
  if (!f.pointers) return {1, VGICP_ERR_BAD_ARGUMENT, align ? "NULL pointer: guess, levels, params and out_pose are required" : "written is NULL"};
  if (build && (f.levels < 0 || f.levels > VGICP_LEVELS_MAX)) return {2, VGICP_ERR_BAD_ARGUMENT, "levels must be 0 .. VGICP_LEVELS_MAX"};
  if (!build && !align && (f.level < 0 || f.level > VGICP_LEVELS_MAX)) return {2, VGICP_ERR_BAD_ARGUMENT, "level must be 0 .. VGICP_LEVELS_MAX"};
  if (align && (f.stages < 1 || f.stages > VGICP_LEVEL_STAGES_MAX)) return {2, VGICP_ERR_BAD_ARGUMENT, "stages must be 1 .. VGICP_LEVEL_STAGES_MAX"};
  if (align && (f.stage_level_min < 0 || f.stage_level_max > VGICP_LEVELS_MAX))
    return {2, VGICP_ERR_BAD_ARGUMENT, "a stage's level must be 0 .. VGICP_LEVELS_MAX"};
  if (!build && !align && f.level > f.requested)
    return {3, VGICP_ERR_NOT_READY, "level is above the number of levels asked for: call vgicp_map_levels_build first"};
  if (align && f.stage_level_max > f.requested)
    return {3, VGICP_ERR_NOT_READY, "a stage's level is above the number of levels asked for: call vgicp_map_levels_build first"};
  if (align && !f.guess_finite) return {4, VGICP_ERR_BAD_ARGUMENT, "an entry of guess is not finite"};
  if (align && f.bad_params_stage >= 0) return {5, VGICP_ERR_BAD_ARGUMENT, ": max_iteration < 0"};   // behind "stage <bad_params_stage>"
  if (f.at.several_devices)
    return {6, VGICP_ERR_BAD_ARGUMENT, "map levels are not available on multi-device contexts, communicators "
                                       "and peer-connected contexts: the resident scan of a device is a shard there"};
  if (!align) {
    if (!f.at.has_map) return {7, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first"};
    if (f.entry == LevelsEntry::Export && f.something_to_write && !f.arrays) return {8, VGICP_ERR_BAD_ARGUMENT, "NULL array pointer"};
    return {};
  }
  LevelsVerdict v = plan_ready(f.at, 7);   // a map, a scan, and after settling still a scan: all rule 7 here
  if (v.rule != 0) v.rule = 7;
  return v;
}

}  // namespace vgicp
