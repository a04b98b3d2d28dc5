// CPU check of what the map levels decide before they touch the device (eskf_lio_amd/csrc/vgicp_levels_plan.h): the
// refusals of the four entry points of include/vgicp_hip_map_levels.h in the header's order, over every combination of
// their facts — the first rule that applies is the one reported — and the sizing of a level's table.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "vgicp_levels_plan.h"

using namespace vgicp;

int main() {
  unsigned long long checks = 0, by_rule[9] = {0};
  const LevelsEntry entries[] = {LevelsEntry::Build, LevelsEntry::Size, LevelsEntry::Export, LevelsEntry::Align};
  const int64_t numbers[] = {-1, 0, 1, 2, 4, 5};         // levels / level / a stage's level
  const uint64_t stage_counts[] = {0, 1, 4, 8, 9};
  for (const LevelsEntry e : entries)
    for (uint32_t bits = 0; bits < 1024; ++bits)
      for (const int64_t number : numbers)
        for (const uint64_t stages : stage_counts)
          for (int requested = 0; requested <= VGICP_LEVELS_MAX; requested += 2) {
            const bool align = e == LevelsEntry::Align, build = e == LevelsEntry::Build, exporting = e == LevelsEntry::Export;
            if (!align && stages != 1) continue;   // the other entries have no stages
            LevelsFacts f;
            f.entry = e;
            f.ctx = bits & 1u;
            f.pointers = (bits >> 1) & 1u;
            f.guess_finite = (bits >> 2) & 1u;
            f.bad_params_stage = ((bits >> 3) & 1u) ? 2 : -1;
            f.at.several_devices = (bits >> 4) & 1u;
            f.at.has_map = (bits >> 5) & 1u;
            f.at.scan_resident = (bits >> 6) & 1u;
            f.at.settled = (bits >> 7) & 1u;
            f.arrays = (bits >> 8) & 1u;
            f.something_to_write = (bits >> 9) & 1u;
            f.levels = f.level = number;
            f.stages = stages;
            f.stage_level_min = number < 0 ? number : 0;   // a schedule from level 0 (or a negative one) up to `number`
            f.stage_level_max = number;
            f.requested = requested;
            const bool in_range = number >= 0 && number <= VGICP_LEVELS_MAX;
            int want = 0;
            if (!f.ctx) want = 1;
            else if (!f.pointers) want = 1;
            else if (align && (stages < 1 || stages > VGICP_LEVEL_STAGES_MAX)) want = 2;
            else if (!in_range) want = 2;
            else if (!build && number > requested) want = 3;
            else if (align && !f.guess_finite) want = 4;
            else if (align && f.bad_params_stage >= 0) want = 5;
            else if (f.at.several_devices) want = 6;
            else if (!f.at.has_map) want = 7;
            else if (align && !f.at.scan_resident) want = 7;
            else if (exporting && f.something_to_write && !f.arrays) want = 8;
            const int status = want == 0 ? VGICP_OK : (want == 3 || want == 7) ? VGICP_ERR_NOT_READY : VGICP_ERR_BAD_ARGUMENT;
            const LevelsVerdict v = plan_levels(f);
            ++checks;
            ++by_rule[v.rule >= 0 && v.rule < 9 ? v.rule : 0];
            bool ok = v.rule == want && v.status == status;
            if (want != 0 && f.ctx) ok = ok && v.text != nullptr;        // a NULL context has nowhere to leave a text
            if (want == 0) ok = ok && v.text == nullptr;
            if (ok && want == 6) ok = std::strstr(v.text, "multi-device contexts, communicators and peer-connected contexts: the resident scan "
                                                          "of a device is a shard there") != nullptr;
            if (ok && want == 7) ok = std::strstr(v.text, f.at.has_map ? "no scan resident" : "no voxel map") != nullptr;
            if (ok && want == 3) ok = std::strstr(v.text, "vgicp_map_levels_build") != nullptr;
            if (!ok) {
              std::printf("MISMATCH: entry %d bits %u number %lld stages %llu requested %d -> rule %d status %d, expected rule %d status %d\n",
                          (int)e, bits, (long long)number, (unsigned long long)stages, requested, v.rule, v.status, want, status);
              return 1;
            }
          }
  // a level's table: a power of two, never below the map table's minimum, at least twice the map's voxels (so that at
  // least half of the slots of EVERY level stay EMPTY), and less than four times above the minimum
  for (uint64_t voxels : {0ull, 1ull, 511ull, 512ull, 513ull, 29154ull, 1000000ull, (1ull << 31) - 1, 1ull << 31}) {
    const uint64_t s = level_slots(voxels);
    ++checks;
    if ((s & (s - 1)) != 0 || s < kMinSlots || s < 2 * voxels || (s > kMinSlots && s >= 4 * voxels) || s > kMaxSlots) {
      std::printf("MISMATCH: level_slots(%llu) = %llu\n", (unsigned long long)voxels, (unsigned long long)s);
      return 1;
    }
  }
  // the voxel size of a level: exactly 2^l times the map's
  for (double h : {0.05, 0.3, 1.0, 7.0})
    for (int l = 0; l <= VGICP_LEVELS_MAX; ++l) {
      ++checks;
      if (level_voxel_size(h, l) != h * (double)(1 << l)) {
        std::printf("MISMATCH: level_voxel_size(%g, %d)\n", h, l);
        return 1;
      }
    }
  std::printf("ok %llu checks:", checks);
  for (int r = 1; r <= 8; ++r) std::printf(" rule %d %llu", r, by_rule[r]);
  std::printf(" passed %llu\n", by_rule[0]);
  return 0;
}
