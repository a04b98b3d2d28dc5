// CPU check of what a carving call refuses before it touches the device (eskf_lio_amd/csrc/vgicp_map_plan.h, plan_carve):
// rules 3 to 9 of include/vgicp_hip_map_carve.h in the header's order, over every combination of their facts — the first
// rule that applies is the one reported — and the bounds of margin, max_range, min_hits and stride at their edges.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "vgicp_map_plan.h"

using namespace vgicp;

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double voxel = 0.5;
  // value, in range
  const struct { double v; bool ok; } margins[] = {{0.0, true}, {-0.0, true}, {0.5, true}, {1e300, true}, {nan, false},
                                                   {-1e-300, false}, {-1.0, false}, {inf, false}, {-inf, false}};
  const struct { double v; bool ok; } ranges[] = {{60.0, true}, {4096.0 * voxel, true}, {1e-300, true}, {std::nextafter(4096.0 * voxel, inf), false},
                                                  {0.0, false}, {-0.0, false}, {-1.0, false}, {nan, false}, {inf, false}, {-inf, false}};
  const struct { uint32_t hits, stride; bool ok; } counts[] = {{1, 1, true}, {5, 3, true}, {0xFFFFFFFFu, 0xFFFFFFFFu, true},
                                                               {0, 1, false}, {1, 0, false}, {0, 0, false}};
  unsigned long long checks = 0, by_rule[10] = {0};
  for (uint32_t bits = 0; bits < 32; ++bits)
    for (const auto& m : margins)
      for (const auto& r : ranges)
        for (const auto& c : counts) {
          CarveFacts f;
          f.has_map = bits & 1u;
          f.scan_resident = (bits >> 1) & 1u;
          f.pointers = (bits >> 2) & 1u;
          f.entries_finite = (bits >> 3) & 1u;
          f.several_devices = (bits >> 4) & 1u;
          f.margin = m.v;
          f.max_range = r.v;
          f.voxel_size = voxel;
          f.min_hits = c.hits;
          f.stride = c.stride;
          const int want = !f.has_map ? 3 : !f.scan_resident ? 3 : !f.pointers ? 4 : !f.entries_finite ? 5 : !m.ok ? 6 : !r.ok ? 7
                           : !c.ok ? 8 : f.several_devices ? 9 : 0;
          const int status = want == 0 ? VGICP_OK : want == 3 ? VGICP_ERR_NOT_READY : VGICP_ERR_BAD_ARGUMENT;
          const CarveVerdict v = plan_carve(f);
          ++checks;
          ++by_rule[v.rule < 10 ? v.rule : 0];
          bool ok = v.rule == want && v.status == status && (want == 0) == (v.text == nullptr);
          // rule 3 names what is missing; rule 9 says why
          if (want == 3) ok = ok && std::strstr(v.text, f.has_map ? "scan" : "map") != nullptr;
          if (want == 9) ok = ok && std::strstr(v.text, "single-device") != nullptr;
          if (!ok) {
            std::printf("MISMATCH: bits %u margin %g range %g hits %u stride %u -> rule %d status %d, expected rule %d status %d\n",
                        bits, m.v, r.v, c.hits, c.stride, v.rule, v.status, want, status);
            return 1;
          }
        }
  // the step bound scales with the map's voxel: 4096 voxel sizes pass, one ulp more does not
  for (double h : {0.05, 0.3, 1.0, 7.0}) {
    CarveFacts f;
    f.has_map = f.scan_resident = f.pointers = f.entries_finite = true;
    f.min_hits = f.stride = 1;
    f.voxel_size = h;
    f.max_range = 4096.0 * h;
    const bool at = plan_carve(f).rule == 0;
    f.max_range = std::nextafter(4097.0 * h, inf);
    const bool beyond = plan_carve(f).rule == 7;
    ++checks;
    if (!at || !beyond) {
      std::printf("MISMATCH: step bound at voxel %g\n", h);
      return 1;
    }
  }
  std::printf("ok %llu verdicts:", checks);
  for (int r = 3; r <= 9; ++r) std::printf(" rule %d %llu", r, by_rule[r]);
  std::printf(" passed %llu\n", by_rule[0]);
  return 0;
}
