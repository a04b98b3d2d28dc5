// vgicp_points_plan.h — what vgicp_points_resident (include/vgicp_hip_points.h) decides without the device: what it
// refuses, in its order; the rank of a quantile; the sort key of a value.  Pure functions of plain facts (no HIP call,
// no context), so that a CPU program can enumerate them (tests/native/points_plan.cpp).  quantile_rank and the keys are
// also what the kernels call (vgicp_kernels.hip): the rank expression is evaluated in this one place.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/vgicp_hip.h"
#include "vgicp_resident_plan.h"

#if defined(__HIPCC__)
#define VGICP_POINTS_FN __host__ __device__ inline
#else
#define VGICP_POINTS_FN inline
#endif

namespace vgicp {

constexpr uint64_t kPointQuantilesMax = 16;   // VGICP_POINT_QUANTILES_MAX

// ---- what the call refuses.  Rules 1-9 are decided before anything is settled, rule 9 once more and rule 10 after
// (`settled`): n is known only then ----
struct PointsFacts : ResidentFacts {   // several_devices, has_map, scan_resident, settled, n: as every call over the resident scan
  bool ctx = true;              // not NULL
  bool same_build = true;       // the context's layout stamp is this build's
  bool pose = true;             // not NULL
  bool pose_finite = true;
  uint64_t n_quantiles = 0;
  bool q = true;                // not NULL
  bool summary = true;          // not NULL
  bool q_in_range = true;       // every q[j] in [0, 1] (a NaN is not)
  bool any_array = false;       // one of d2 / sq_error / weight / status is given
  uint64_t capacity = 0;
};
struct PointsVerdict {
  int status = VGICP_OK;
  int rule = 0;                 // 1 .. 10 of the header's list; 0: not refused
  const char* text = nullptr;   // status != VGICP_OK (rules 1 and 2 have no context to leave it in)
  bool sets_points = false;     // rule 10: summary->points = n is written all the same
};
inline PointsVerdict plan_points(const PointsFacts& f) {
  const auto refuse = [](int rule, int status, const char* text) { return PointsVerdict{status, rule, text, rule == 10}; };
  if (!f.ctx) return refuse(1, VGICP_ERR_BAD_ARGUMENT, "NULL context");
  if (!f.same_build)
    return refuse(2, VGICP_ERR_BAD_ARGUMENT,
                  "libvgicp_hip_points.so and the libvgicp_hip.so that created this context are not from one build");
  if (!f.pose) return refuse(3, VGICP_ERR_BAD_ARGUMENT, "NULL pose");
  if (!f.pose_finite) return refuse(4, VGICP_ERR_BAD_ARGUMENT, "the pose has an entry that is not finite");
  if (f.n_quantiles > kPointQuantilesMax) return refuse(5, VGICP_ERR_BAD_ARGUMENT, "n_quantiles must be 0 .. VGICP_POINT_QUANTILES_MAX");
  if (f.n_quantiles > 0 && (!f.q || !f.summary)) return refuse(6, VGICP_ERR_BAD_ARGUMENT, "quantiles need q and summary");
  if (f.n_quantiles > 0 && !f.q_in_range) return refuse(7, VGICP_ERR_BAD_ARGUMENT, "a quantile is not in [0, 1]");
  if (f.several_devices)
    return refuse(8, VGICP_ERR_BAD_ARGUMENT,
                  "vgicp_points_resident is not available on multi-device contexts, communicators "
                  "and peer-connected contexts: the resident scan of a device is a shard there");
  if (!f.has_map) return refuse(9, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (!f.scan_resident) return refuse(9, VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  if (f.settled && f.any_array && f.capacity < f.n) return refuse(10, VGICP_ERR_BAD_ARGUMENT, "capacity smaller than the resident scan");
  return PointsVerdict{};
}

// ---- the rank of quantile q among m ranked values, ascending from 0: min(max(ceil(q m), 1), m) - 1 in fp64 (the
// product is one rounding, ceil is exact; m < 2^53).  THE definition: the pick kernel calls this.  m = 0 has no rank
// (the caller reports NaN); 0 is returned ----
VGICP_POINTS_FN uint64_t quantile_rank(double q, uint64_t m) {
  if (m == 0) return 0;
  const double dm = (double)m;
  double r = __builtin_ceil(q * dm);
  r = r > 1.0 ? r : 1.0;        // also takes a NaN to 1
  r = r < dm ? r : dm;
  return (uint64_t)r - 1u;
}

// ---- sort keys: the bit pattern of max(value, 0), which is monotone for non-negative doubles (+0 for a negative value
// and for -0); a point that is not ranked (not matched, or a raw that is not finite) sorts behind every value.  The
// library's sort (vgicp_sort.h) wants every key below ~0 ----
constexpr uint64_t kPointKeyUnranked = 0xFFFFFFFFFFFFFFFEull;
VGICP_POINTS_FN uint64_t point_key(double value) {
  const double d2 = value > 0.0 ? value : 0.0;
  uint64_t k;
  __builtin_memcpy(&k, &d2, sizeof k);
  return k;
}
VGICP_POINTS_FN double point_key_value(uint64_t key) {
  double v;
  __builtin_memcpy(&v, &key, sizeof v);
  return v;
}

}  // namespace vgicp
