// vgicp_map_plan.h — what a map update decides before it touches the device: how large the voxel table and the raw-point
// log are made and when they grow, whether an insertion goes without its sort, and what each insertion entry point
// refuses, in its own order.  Pure functions of plain facts (no HIP call, no context), so that a CPU program can
// enumerate them (tests/native/map_plan.cpp).  DESIGN.md §4 "Where a map update is decided".
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/vgicp_hip.h"
#include "vgicp_resident_plan.h"

namespace vgicp {

constexpr uint64_t kMinSlots = 1024;
constexpr uint64_t kMaxSlots = 1ull << 32;        // slot indices are 32-bit
constexpr uint64_t kRawMinEntries = 4096;
constexpr uint64_t kRawMaxEntries = 1ull << 31;   // 64 GiB of raw points; ordinals and offsets stay 32-bit

inline uint64_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// ---- the voxel table: load (FULL + TOMB + incoming + a pending insertion's upper bound) <= 1/2 at all times; a new
// table is sized for load <= 1/4 ----
struct TableGrowth {
  bool grow = false;
  uint64_t slots = 0;        // of the new table (grow only)
  bool too_large = false;    // ... which would exceed 2^32 slots: refused
};
inline TableGrowth table_for(uint64_t entries) {
  TableGrowth g;
  g.grow = true;
  g.slots = next_pow2(std::max<uint64_t>(kMinSlots, entries * 4));
  g.too_large = g.slots > kMaxSlots;
  return g;
}
// vgicp_map_reset: 4 slots per voxel hinted
inline TableGrowth plan_first_table(uint64_t capacity_hint) { return table_for(capacity_hint); }
inline TableGrowth plan_table_growth(bool has_table, uint64_t slots, uint64_t voxels, uint64_t tombstones,
                                     uint64_t pending_upper, uint64_t incoming) {
  const uint64_t used = voxels + tombstones + incoming + pending_upper;
  if (has_table && used * 2 <= slots) return TableGrowth{};
  return table_for(voxels + incoming);   // the tombstones stay behind; a pending insertion has been settled by then
}

// ---- the raw-point log: sized from the hint like the table (4 entries per voxel hinted); when the bound says an
// insertion could fill it, the live entries are compacted and the log doubles until it is twice what is needed ----
inline uint64_t plan_first_raw_log(uint64_t capacity_hint) {
  return std::min(kRawMaxEntries, next_pow2(std::max<uint64_t>(kRawMinEntries, capacity_hint * 4)));
}
inline bool raw_log_needs_compaction(uint64_t used_upper, uint64_t incoming, uint64_t capacity) {
  return used_upper + incoming > capacity;
}
struct RawGrowth {
  uint64_t capacity = 0;     // of the log the live entries move to (== the current one: compacted in place of it)
  bool too_large = false;    // live + incoming do not fit 2^31 entries: refused
};
inline RawGrowth plan_raw_growth(uint64_t live, uint64_t incoming, uint64_t capacity) {
  RawGrowth g;
  g.capacity = capacity;
  while (g.capacity < kRawMaxEntries && 2 * (live + incoming) > g.capacity) g.capacity *= 2;
  g.too_large = live + incoming > g.capacity;
  return g;
}

// A scan the device down-sampled itself holds one point per voxel of ITS grid: a voxel of the map then receives at
// most (map voxel / scan voxel + 1)^3 of them, and when that is a handful the insertion goes without its sort
// (launch_map_insert, short_lists).  Any other scan (uploaded as it came: scan_voxel 0) keeps the sort.
inline bool insertion_lists_stay_short(double map_voxel, double scan_voxel, bool insert_sort) {
  if (!(scan_voxel > 0.0) || insert_sort) return false;
  const double per_axis = std::ceil(map_voxel / scan_voxel) + 1.0;
  return per_axis * per_axis * per_axis <= 64.0;
}

// ---- what an insertion entry point refuses.  The four entries check in different orders and not all the same things;
// each order is kept as it was written (DESIGN.md has the table) ----
enum class InsertEntry {
  Scan,            // vgicp_map_insert_scan: the scan comes from host buffers
  Resident,        // vgicp_map_insert_resident
  ResidentAsync,   // vgicp_map_insert_resident_async
  Device,          // vgicp_internal::map_insert_device: a multi-device context's replica, the scan is on its device
  // include/vgicp_hip_map_gated.h: the resident entries' checks in the resident entries' order; what a gated entry
  // refuses beyond them (transform entries, the gate, several devices, capacity) follows in plan_gate below
  ResidentGated,       // vgicp_map_insert_resident_gated
  ResidentGatedAsync   // vgicp_map_insert_resident_gated_async
};
struct InsertFacts {
  InsertEntry entry = InsertEntry::Scan;
  bool has_table = false;
  bool scan_resident = false;   // Resident, ResidentAsync
  bool pointers = false;        // every pointer the entry takes is there (Scan: points, covs, transform; else: transform)
  uint64_t points_per_voxel = 0;
  bool raw_on = false;
  uint64_t n = 0;               // ResidentAsync: known only once the entry has settled; no refusal of its depends on n
  bool shard_only = false;      // the resident scan is one rank's shard (Resident, ResidentAsync)
};
struct InsertVerdict {
  int status = VGICP_OK;
  const char* text = nullptr;   // status != VGICP_OK
  bool nothing_to_do = false;   // status == VGICP_OK and n == 0: the entry returns without touching the map
};

inline InsertVerdict plan_insert(const InsertFacts& f) {
  const auto refuse = [](int status, const char* text) { return InsertVerdict{status, text, false}; };
  const InsertVerdict nothing{VGICP_OK, nullptr, true};
  const bool resident = f.entry == InsertEntry::Resident || f.entry == InsertEntry::ResidentAsync ||
                        f.entry == InsertEntry::ResidentGated || f.entry == InsertEntry::ResidentGatedAsync;
  if (!f.has_table) return refuse(VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (f.entry == InsertEntry::Scan && f.n == 0) return nothing;   // before it looks at a pointer
  if (resident && !f.scan_resident) return refuse(VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  if (!f.pointers) return refuse(VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  if (f.points_per_voxel == 0) return refuse(VGICP_ERR_BAD_ARGUMENT, "max_points_per_voxel must be >= 1");
  if (f.raw_on && f.points_per_voxel > 0xFFFFFFFFull)
    return refuse(VGICP_ERR_BAD_ARGUMENT, "max_points_per_voxel must be < 2^32 while the map keeps raw points");
  if (resident && f.shard_only)
    return refuse(VGICP_ERR_BAD_ARGUMENT, "resident scan is a shard: use vgicp_map_insert_scan with the whole scan");
  if (!resident && f.n > 0x7FFFFFFFull) return refuse(VGICP_ERR_BAD_ARGUMENT, "scan too large");   // (the resident entries never had this check)
  return f.n == 0 ? nothing : InsertVerdict{};
}

// ---- what a gated insertion refuses once plan_insert has passed (include/vgicp_hip_map_gated.h, rules 4 to 7) ----
struct GateFacts : ResidentFacts {   // several_devices and n are asked here: plan_insert has asked for the map and the scan
  bool transform_finite = false;
  double gate = 0.0;
  bool kept_given = false;        // the synchronous entry, once settled: the caller's keep array ...
  uint64_t capacity = 0;          // ... and its length
};
struct GateVerdict {
  int rule = 0;                   // 0: passed, else the header's number
  int status = VGICP_OK;
  const char* text = nullptr;
};
// finite and >= 0, or +inf
inline bool gate_in_range(double gate) { return gate >= 0.0; }
inline GateVerdict plan_gate(const GateFacts& f) {
  if (!f.transform_finite) return GateVerdict{4, VGICP_ERR_BAD_ARGUMENT, "a transform entry is not finite"};
  if (!gate_in_range(f.gate)) return GateVerdict{5, VGICP_ERR_BAD_ARGUMENT, "gate must be finite and >= 0, or +infinity"};
  if (f.several_devices)
    return GateVerdict{6, VGICP_ERR_BAD_ARGUMENT, "gated insertion works on a single-device context: the resident scan of a device is a shard here"};
  if (f.kept_given && f.capacity < f.n) return GateVerdict{7, VGICP_ERR_BAD_ARGUMENT, "kept holds fewer than the scan's points"};
  return GateVerdict{};
}

// ---- what a carving call refuses (include/vgicp_hip_map_carve.h, rules 3 to 9; 1 and 2 are the side library's
// handshake).  The two entries refuse alike: nothing here depends on the scan's size ----
struct CarveFacts : ResidentFacts {   // has_map, scan_resident, several_devices
  bool pointers = false;          // transform and params are there
  bool entries_finite = false;    // all 16 of the transform and the 3 of the origin
  double margin = 0.0, max_range = 0.0, voxel_size = 0.0;
  uint32_t min_hits = 0, stride = 0;
};
using CarveVerdict = GateVerdict;
constexpr double kCarveMaxSteps = 4096.0;   // VGICP_CARVE_MAX_STEPS: a ray's walk is bounded by 3 (this + 1) + 3 steps
inline CarveVerdict plan_carve(const CarveFacts& f) {
  if (!f.has_map) return CarveVerdict{3, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first"};
  if (!f.scan_resident) return CarveVerdict{3, VGICP_ERR_NOT_READY, kNoScanText};
  if (!f.pointers) return CarveVerdict{4, VGICP_ERR_BAD_ARGUMENT, "NULL pointer"};
  if (!f.entries_finite) return CarveVerdict{5, VGICP_ERR_BAD_ARGUMENT, "a transform or origin entry is not finite"};
  if (!(f.margin >= 0.0) || std::isinf(f.margin)) return CarveVerdict{6, VGICP_ERR_BAD_ARGUMENT, "margin must be finite and >= 0"};
  if (!(f.max_range > 0.0) || std::isinf(f.max_range) || !(f.max_range / f.voxel_size <= kCarveMaxSteps))
    return CarveVerdict{7, VGICP_ERR_BAD_ARGUMENT, "max_range must be finite, > 0 and at most 4096 voxel sizes"};
  if (f.min_hits == 0 || f.stride == 0) return CarveVerdict{8, VGICP_ERR_BAD_ARGUMENT, "min_hits and stride must be >= 1"};
  if (f.several_devices)
    return CarveVerdict{9, VGICP_ERR_BAD_ARGUMENT, "carving works on a single-device context: the resident scan of a device is a shard here"};
  return CarveVerdict{};
}

// ---- what the ray report refuses (include/vgicp_hip_map_rays.h, rules 3 to 11; 1 and 2 are the side library's
// handshake), and how its poses go in groups ----
struct RayFacts : ResidentFacts {   // has_map, scan_resident, several_devices
  bool pointers = false;          // poses and params are there
  uint64_t n_poses = 0;
  bool entries_finite = false;    // all 16 of every pose and the 3 of the origin
  double margin = 0.0, beyond = 0.0, max_range = 0.0, voxel_size = 0.0;
  uint32_t stride = 0, reserved = 0;
  bool per_point = false;         // a per-point plane is asked for
};
using RayVerdict = GateVerdict;
constexpr uint64_t kRayMaxPoses = 64;                 // VGICP_RAYS_MAX_POSES
constexpr uint64_t kRayBitmapBudget = 16ull << 20;    // bytes of confirmation bitmaps one group of poses may take
inline RayVerdict plan_rays(const RayFacts& f) {
  if (!f.has_map) return RayVerdict{3, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first"};
  if (!f.scan_resident) return RayVerdict{3, VGICP_ERR_NOT_READY, kNoScanText};
  if (!f.pointers || f.n_poses == 0 || f.n_poses > kRayMaxPoses)
    return RayVerdict{4, VGICP_ERR_BAD_ARGUMENT, "poses and params must not be NULL, n_poses 1 .. VGICP_RAYS_MAX_POSES"};
  if (!f.entries_finite) return RayVerdict{5, VGICP_ERR_BAD_ARGUMENT, "a pose or origin entry is not finite"};
  if (!(f.margin >= 0.0) || std::isinf(f.margin)) return RayVerdict{6, VGICP_ERR_BAD_ARGUMENT, "margin must be finite and >= 0"};
  if (!(f.beyond >= 0.0) || std::isinf(f.beyond)) return RayVerdict{7, VGICP_ERR_BAD_ARGUMENT, "beyond must be finite and >= 0"};
  if (!(f.max_range > 0.0) || std::isinf(f.max_range) || !(f.max_range / f.voxel_size <= kCarveMaxSteps))
    return RayVerdict{8, VGICP_ERR_BAD_ARGUMENT, "max_range must be finite, > 0 and at most 4096 voxel sizes"};
  if (f.stride == 0 || f.reserved != 0) return RayVerdict{9, VGICP_ERR_BAD_ARGUMENT, "stride must be >= 1 and reserved 0"};
  if (f.per_point && f.n_poses != 1) return RayVerdict{10, VGICP_ERR_BAD_ARGUMENT, "per-point outputs are for a single pose"};
  if (f.several_devices)
    return RayVerdict{11, VGICP_ERR_BAD_ARGUMENT, "the ray report works on a single-device context: the resident scan of a device is a shard here"};
  return RayVerdict{};
}
// one bit per slot and pose (slots: a power of two >= kMinSlots, so whole 32-bit words); the poses one group holds
inline uint64_t ray_bitmap_bytes(uint64_t slots) { return slots / 8; }
inline uint64_t ray_group_poses(uint64_t slots) {
  return std::max<uint64_t>(1, std::min<uint64_t>(kRayMaxPoses, kRayBitmapBudget / std::max<uint64_t>(1, ray_bitmap_bytes(slots))));
}
inline uint64_t ray_groups(uint64_t slots, uint64_t n_poses) {
  const uint64_t per = ray_group_poses(slots);
  return (n_poses + per - 1) / per;
}

}  // namespace vgicp
