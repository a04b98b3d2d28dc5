// CPU check of what the ray report refuses before it touches the device (eskf_lio_amd/csrc/vgicp_map_plan.h, plan_rays):
// rules 3 to 11 of include/vgicp_hip_map_rays.h in the header's order, over every combination of their facts — the first
// rule that applies is the one reported — the bounds of margin, beyond, max_range, stride and n_poses at their edges, and
// how the poses go in groups.
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
  const struct { double v; bool ok; } lengths[] = {{0.0, true}, {-0.0, true}, {1.0, true}, {1e300, true}, {nan, false},
                                                   {-1e-300, false}, {inf, false}, {-inf, false}};
  const struct { double v; bool ok; } ranges[] = {{60.0, true}, {4096.0 * voxel, true}, {1e-300, true}, {std::nextafter(4096.0 * voxel, inf), false},
                                                  {0.0, false}, {-1.0, false}, {nan, false}, {inf, false}};
  const struct { uint32_t stride, reserved; bool ok; } words[] = {{1, 0, true}, {3, 0, true}, {0xFFFFFFFFu, 0, true},
                                                                  {0, 0, false}, {1, 1, false}, {0, 7, false}};
  const struct { uint64_t n; bool ok; } poses[] = {{1, true}, {2, true}, {64, true}, {0, false}, {65, false}, {~0ull, false}};
  unsigned long long checks = 0, by_rule[12] = {0};
  for (uint32_t bits = 0; bits < 64; ++bits)
    for (const auto& m : lengths)
      for (const auto& b : lengths)
        for (const auto& r : ranges)
          for (const auto& w : words)
            for (const auto& k : poses) {
              RayFacts f;
              f.has_map = bits & 1u;
              f.scan_resident = (bits >> 1) & 1u;
              f.pointers = (bits >> 2) & 1u;
              f.entries_finite = (bits >> 3) & 1u;
              f.several_devices = (bits >> 4) & 1u;
              f.per_point = (bits >> 5) & 1u;
              f.n_poses = k.n;
              f.margin = m.v;
              f.beyond = b.v;
              f.max_range = r.v;
              f.voxel_size = voxel;
              f.stride = w.stride;
              f.reserved = w.reserved;
              const int want = !f.has_map ? 3 : !f.scan_resident ? 3 : (!f.pointers || !k.ok) ? 4 : !f.entries_finite ? 5 : !m.ok ? 6
                               : !b.ok ? 7 : !r.ok ? 8 : !w.ok ? 9 : (f.per_point && k.n != 1) ? 10 : f.several_devices ? 11 : 0;
              const int status = want == 0 ? VGICP_OK : want == 3 ? VGICP_ERR_NOT_READY : VGICP_ERR_BAD_ARGUMENT;
              const RayVerdict v = plan_rays(f);
              ++checks;
              ++by_rule[v.rule < 12 ? v.rule : 0];
              bool ok = v.rule == want && v.status == status && (want == 0) == (v.text == nullptr);
              // rule 3 names what is missing; rule 11 says why
              if (want == 3) ok = ok && std::strstr(v.text, f.has_map ? "scan" : "map") != nullptr;
              if (want == 11) ok = ok && std::strstr(v.text, "single-device") != nullptr;
              if (!ok) {
                std::printf("MISMATCH: bits %u margin %g beyond %g range %g stride %u reserved %u poses %llu -> rule %d status %d, expected rule %d status %d\n",
                            bits, m.v, b.v, r.v, w.stride, w.reserved, (unsigned long long)k.n, v.rule, v.status, want, status);
                return 1;
              }
            }
  // the step bound scales with the map's voxel: 4096 voxel sizes pass, more does not
  for (double h : {0.05, 0.3, 1.0, 7.0}) {
    RayFacts f;
    f.has_map = f.scan_resident = f.pointers = f.entries_finite = true;
    f.n_poses = f.stride = 1;
    f.voxel_size = h;
    f.max_range = 4096.0 * h;
    const bool at = plan_rays(f).rule == 0;
    f.max_range = std::nextafter(4097.0 * h, inf);
    const bool beyond = plan_rays(f).rule == 8;
    ++checks;
    if (!at || !beyond) {
      std::printf("MISMATCH: step bound at voxel %g\n", h);
      return 1;
    }
  }
  // groups: as many poses as fit 16 MiB of bitmaps (slots / 8 bytes each), at least one, at most all 64
  const struct { uint64_t slots, per, poses, groups; } g[] = {
      {1024, 64, 64, 1}, {1ull << 21, 64, 64, 1}, {1ull << 22, 32, 33, 2}, {1ull << 23, 16, 33, 3}, {1ull << 23, 16, 16, 1},
      {1ull << 23, 16, 17, 2}, {1ull << 27, 1, 5, 5}, {1ull << 28, 1, 1, 1}, {1ull << 32, 1, 64, 64}};
  for (const auto& c : g) {
    ++checks;
    if (ray_group_poses(c.slots) != c.per || ray_groups(c.slots, c.poses) != c.groups || ray_bitmap_bytes(c.slots) * 8 != c.slots) {
      std::printf("MISMATCH: groups at %llu slots, %llu poses\n", (unsigned long long)c.slots, (unsigned long long)c.poses);
      return 1;
    }
  }
  std::printf("ok %llu checks:", checks);
  for (int r = 3; r <= 11; ++r) std::printf(" rule %d %llu", r, by_rule[r]);
  std::printf(" passed %llu\n", by_rule[0]);
  return 0;
}
