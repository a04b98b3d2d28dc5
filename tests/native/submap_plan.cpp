// CPU check of what vgicp_scan_from_map decides before it touches the device (eskf_lio_amd/csrc/vgicp_submap_plan.h):
// its refusals in the order of include/vgicp_hip_map_submap.h, over every combination of its facts — the first rule that
// applies is the one reported — and the geometry of its launches.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "vgicp_submap_plan.h"

using namespace vgicp;

int main() {
  unsigned long long checks = 0, by_rule[12] = {0};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int64_t levels[] = {-1, 0, 2, 4, 5};
  const double radii[] = {0.0, 2.5, inf, -0.0, -1.0, -inf, nan};
  const uint64_t voxels[] = {0, 1, 0xFFFFFFFFull, 0x100000000ull};
  for (uint32_t bits = 0; bits < (1u << 12); ++bits)
    for (const int64_t level : levels)
      for (const double radius : radii)
        for (const uint64_t v : voxels)
          for (int requested = 0; requested <= VGICP_LEVELS_MAX; requested += 2) {
            SubmapFacts f;
            f.dst = bits & 1u;
            f.src = (bits >> 1) & 1u;
            f.params = (bits >> 2) & 1u;
            f.dst_build = (bits >> 3) & 1u;
            f.src_build = (bits >> 4) & 1u;
            f.several_devices = (bits >> 5) & 1u;
            f.same_device = (bits >> 6) & 1u;
            f.reserved = (bits >> 7) & 1u ? 0 : 7;
            f.center_finite = (bits >> 8) & 1u;
            f.frame_finite = (bits >> 9) & 1u;
            f.src_has_map = (bits >> 10) & 1u;
            f.settled = (bits >> 11) & 1u;
            f.level = level;
            f.requested = requested;
            f.radius = radius;
            f.voxels = v;
            int want = 0;
            if (!f.dst || !f.src || !f.params) want = 1;
            else if (!f.dst_build || !f.src_build) want = 2;
            else if (f.several_devices) want = 3;
            else if (!f.same_device) want = 4;
            else if (f.reserved != 0) want = 5;
            else if (level < 0 || level > VGICP_LEVELS_MAX) want = 6;
            else if (level > requested) want = 7;
            else if (!f.center_finite || !f.frame_finite) want = 8;
            else if (std::isnan(radius) || (radius < 0.0)) want = 9;
            else if (!f.src_has_map) want = 10;
            else if (f.settled && v > 0xFFFFFFFFull) want = 11;
            const int status = want == 0 ? VGICP_OK : (want == 7 || want == 10) ? VGICP_ERR_NOT_READY : VGICP_ERR_BAD_ARGUMENT;
            const SubmapVerdict got = plan_submap(f);
            ++checks;
            ++by_rule[got.rule >= 0 && got.rule < 12 ? got.rule : 0];
            bool ok = got.rule == want && got.status == status && (want == 0) == (got.text == nullptr);
            const char* word[12] = {"", "NULL pointer", "not from one build", "multi-device contexts, communicators and peer-connected contexts: "
                                    "the resident scan of a device is a shard there", "different devices", "reserved", "level must be",
                                    "vgicp_map_levels_build", "not finite", "radius", "no voxel map", "scan too large"};
            if (ok && want != 0) ok = std::strstr(got.text, word[want]) != nullptr;
            // the entry point's own library asks rules 1 and 2 and nothing else
            const SubmapVerdict hs = plan_submap_handshake(f);
            ok = ok && hs.rule == (want == 1 || want == 2 ? want : 0);
            if (!ok) {
              std::printf("MISMATCH: bits %u level %lld radius %g voxels %llu requested %d -> rule %d status %d, expected rule %d status %d\n",
                          bits, (long long)level, radius, (unsigned long long)v, requested, got.rule, got.status, want, status);
              return 1;
            }
          }
  // the text of a level nobody asked for is locate's
  LocateFacts lf;
  lf.level = 2;
  SubmapFacts sf;
  sf.level = 2;
  if (std::strcmp(plan_locate(lf).text, plan_submap(sf).text) != 0 || plan_locate(lf).status != plan_submap(sf).status) {
    std::printf("MISMATCH: the missing level's wording\n");
    return 1;
  }
  // the groups cover the slots exactly, a group's ballots its slots, and the scratch holds all of it
  for (uint64_t slots : {1ull, 64ull, 1024ull, 1025ull, 4096ull, 2097152ull, 1ull << 32}) {
    const uint64_t g = submap_groups(slots);
    ++checks;
    if (g * kSubmapGroupSlots < slots || (g - 1) * kSubmapGroupSlots >= slots || kSubmapGroupWords * 64 != kSubmapGroupSlots ||
        submap_work_bytes(slots) < g * kSubmapGroupWords * 8 + 3 * g * 4 + 3 * 8 || submap_work_bytes(slots) % 8 != 0) {
      std::printf("MISMATCH: submap_groups(%llu) = %llu\n", (unsigned long long)slots, (unsigned long long)g);
      return 1;
    }
  }
  std::printf("ok %llu checks:", checks);
  for (int r = 1; r <= 11; ++r) std::printf(" rule %d %llu", r, by_rule[r]);
  std::printf(" passed %llu\n", by_rule[0]);
  return 0;
}
