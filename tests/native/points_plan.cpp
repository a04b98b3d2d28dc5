// What vgicp_points_resident decides without the device (eskf_lio_amd/csrc/vgicp_points_plan.h), on the CPU:
//   - plan_points over every combination of its facts against the header's numbered list, restated here as a list of
//     predicates taken in order (the first that holds names the rule);
//   - quantile_rank for the sizes and quantiles tests/test_points_cpu.py names, printed for the test to hold against the
//     formula in Python integers;
//   - the sort key: monotone over an ascending list of doubles, +0 for everything that is not positive, the unranked
//     key above every value and below ~0, and the value back from the key.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "vgicp_points_plan.h"

using namespace vgicp;

namespace {
// include/vgicp_hip_points.h, REFUSALS: (rule, status) of the first line that applies; 0 = not refused
struct Want { int rule, status; };
Want by_the_list(const PointsFacts& f) {
  if (!f.ctx) return {1, VGICP_ERR_BAD_ARGUMENT};
  if (!f.same_build) return {2, VGICP_ERR_BAD_ARGUMENT};
  if (!f.pose) return {3, VGICP_ERR_BAD_ARGUMENT};
  if (!f.pose_finite) return {4, VGICP_ERR_BAD_ARGUMENT};
  if (f.n_quantiles > 16) return {5, VGICP_ERR_BAD_ARGUMENT};
  if (f.n_quantiles > 0 && !(f.q && f.summary)) return {6, VGICP_ERR_BAD_ARGUMENT};
  if (f.n_quantiles > 0 && !f.q_in_range) return {7, VGICP_ERR_BAD_ARGUMENT};
  if (f.several_devices) return {8, VGICP_ERR_BAD_ARGUMENT};
  if (!f.has_map || !f.scan_resident) return {9, VGICP_ERR_NOT_READY};
  if (f.settled && f.any_array && f.capacity < f.n) return {10, VGICP_ERR_BAD_ARGUMENT};
  return {0, VGICP_OK};
}
}  // namespace

int main() {
  // ---- the refusal order ----
  const uint64_t quantiles[] = {0, 1, 16, 17};
  const uint64_t sizes[][2] = {{0, 0}, {5, 6}, {6, 6}, {7, 6}, {0, 6}};   // capacity, n
  unsigned long long checked = 0, seen[11] = {0};
  for (unsigned bits = 0; bits < (1u << 12); ++bits)
    for (uint64_t nq : quantiles)
      for (const auto& cn : sizes) {
        PointsFacts f;
        f.ctx = bits & 1u; f.same_build = bits & 2u; f.pose = bits & 4u; f.pose_finite = bits & 8u;
        f.q = bits & 16u; f.summary = bits & 32u; f.q_in_range = bits & 64u; f.several_devices = bits & 128u;
        f.has_map = bits & 256u; f.scan_resident = bits & 512u; f.settled = bits & 1024u; f.any_array = bits & 2048u;
        f.n_quantiles = nq; f.capacity = cn[0]; f.n = cn[1];
        const PointsVerdict v = plan_points(f);
        const Want w = by_the_list(f);
        const bool text_ok = (v.status == VGICP_OK) == (v.text == nullptr);
        if (v.rule != w.rule || v.status != w.status || !text_ok || v.sets_points != (w.rule == 10)) {
          std::printf("plan_points: facts %u nq %llu capacity %llu n %llu: rule %d status %d, want %d %d\n", bits,
                      (unsigned long long)nq, (unsigned long long)cn[0], (unsigned long long)cn[1], v.rule, v.status, w.rule, w.status);
          return 1;
        }
        ++seen[v.rule];
        ++checked;
      }
  for (int r = 0; r <= 10; ++r)
    if (!seen[r]) { std::printf("plan_points: rule %d never turned up\n", r); return 1; }
  // the text of rule 8 names what vgicp_evaluate_resident's names
  {
    PointsFacts f;
    f.several_devices = true;
    const char* t = plan_points(f).text;
    if (!t || !std::strstr(t, "multi-device contexts, communicators and peer-connected contexts: the resident scan of a device is a shard there")) {
      std::printf("rule 8: text\n");
      return 1;
    }
  }
  std::printf("plan ok %llu\n", checked);

  // ---- quantile_rank ----
  const uint64_t ms[] = {0, 1, 2, 255, 256, 257, 5856, 2147483647ull};
  const double qs[] = {0.0, 1e-12, 0.25, 0.5, 0.9, 0.99, 1.0 - 0x1p-53, 1.0};
  for (uint64_t m : ms)
    for (int j = 0; j < 8; ++j) std::printf("rank %llu %d %llu\n", (unsigned long long)m, j, (unsigned long long)quantile_rank(qs[j], m));
  if (quantile_rank(std::numeric_limits<double>::quiet_NaN(), 7) != 0) { std::printf("rank of NaN\n"); return 1; }

  // ---- keys ----
  const double ascending[] = {0.0, 4.9406564584124654e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1e-3, 1.0,
                              1.0000000000000002, 1.7976931348623157e308};
  const int count = (int)(sizeof ascending / sizeof ascending[0]);
  for (int k = 0; k < count; ++k) {
    const uint64_t key = point_key(ascending[k]);
    double back = point_key_value(key);
    if (std::memcmp(&back, &ascending[k], 8) != 0) { std::printf("key %d does not give its value back\n", k); return 1; }
    if (k && !(point_key(ascending[k - 1]) < key)) { std::printf("keys %d and %d are not in order\n", k - 1, k); return 1; }
    if (!(key < kPointKeyUnranked)) { std::printf("key %d is not below the unranked key\n", k); return 1; }
  }
  if (point_key(0.0) != 0 || point_key(-0.0) != 0 || point_key(-1.0) != 0 || point_key(-1e-300) != 0) { std::printf("keys of non-positive values\n"); return 1; }
  if (!(point_key(std::numeric_limits<double>::infinity()) < kPointKeyUnranked) || !(kPointKeyUnranked < ~0ull)) { std::printf("the unranked key\n"); return 1; }
  std::printf("keys ok\n");
  return 0;
}
