// CPU check of what a gated map insertion refuses before it touches the device (eskf_lio_amd/csrc/vgicp_map_plan.h):
//   * plan_insert for the two gated entries, over every combination of the facts tests/native/map_plan.cpp enumerates:
//     the verdict (status, text, nothing to do) of vgicp_map_insert_resident resp. its _async form — rule 3 of
//     include/vgicp_hip_map_gated.h says "everything vgicp_map_insert_resident refuses, in its order";
//   * the four entries from before, printed as one line per combination, so that the Python test can compare the
//     listing with the one the parent's header gives (the verdicts must not change);
//   * plan_gate: rules 4 to 7 in that order over every combination of their facts, and the gate's range.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "vgicp_map_plan.h"

using namespace vgicp;

static bool same(const InsertVerdict& a, const InsertVerdict& b) {
  const bool text = (a.text == nullptr) == (b.text == nullptr) && (!a.text || std::strcmp(a.text, b.text) == 0);
  return a.status == b.status && text && a.nothing_to_do == b.nothing_to_do;
}

int main(int argc, char** argv) {
  const bool listing = argc > 1 && std::strcmp(argv[1], "list") == 0;
  const uint64_t one = 1;
  const uint64_t ns[] = {0, 1, (one << 31) - 1, one << 31};
  const uint64_t caps[] = {0, 1, (one << 32) - 1, one << 32};
  const InsertEntry old_entries[] = {InsertEntry::Scan, InsertEntry::Resident, InsertEntry::ResidentAsync, InsertEntry::Device};
  unsigned long long checks = 0, refused = 0, nothing = 0;
  for (uint32_t bits = 0; bits < 32; ++bits)
    for (uint64_t n : ns)
      for (uint64_t cap : caps) {
        InsertFacts f;
        f.has_table = bits & 1u;
        f.scan_resident = (bits >> 1) & 1u;
        f.pointers = (bits >> 2) & 1u;
        f.raw_on = (bits >> 3) & 1u;
        f.shard_only = (bits >> 4) & 1u;
        f.n = n;
        f.points_per_voxel = cap;
        if (listing) {
          for (InsertEntry e : old_entries) {
            f.entry = e;
            const InsertVerdict v = plan_insert(f);
            std::printf("%d %u %llu %llu -> %d %d %s\n", (int)e, bits, (unsigned long long)n, (unsigned long long)cap, v.status,
                        (int)v.nothing_to_do, v.text ? v.text : "-");
          }
          continue;
        }
        const InsertEntry pairs[2][2] = {{InsertEntry::ResidentGated, InsertEntry::Resident},
                                         {InsertEntry::ResidentGatedAsync, InsertEntry::ResidentAsync}};
        for (const auto& pair : pairs) {
          f.entry = pair[0];
          const InsertVerdict got = plan_insert(f);
          f.entry = pair[1];
          const InsertVerdict want = plan_insert(f);
          ++checks;
          refused += got.status != VGICP_OK;
          nothing += got.nothing_to_do;
          if (!same(got, want)) {
            std::printf("MISMATCH (gated entry %d): bits %u n %llu cap %llu -> %d '%s'\n", (int)pair[0], bits, (unsigned long long)n,
                        (unsigned long long)cap, got.status, got.text ? got.text : "");
            return 1;
          }
        }
      }
  if (listing) return 0;
  // plan_gate: the first rule that applies, in the header's order
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double gates[] = {0.0, -0.0, 0.04, 1e300, inf, nan, -1e-300, -1.0, -inf};
  unsigned long long gate_checks = 0;
  for (double gate : gates)
    for (uint32_t bits = 0; bits < 16; ++bits) {
      GateFacts g;
      g.transform_finite = bits & 1u;
      g.several_devices = (bits >> 1) & 1u;
      g.kept_given = (bits >> 2) & 1u;
      g.n = 100;
      g.capacity = ((bits >> 3) & 1u) ? 100 : 99;
      g.gate = gate;
      const bool gate_ok = gate >= 0.0;   // NaN, negative, -inf fail; -0.0 is 0
      const int want = !g.transform_finite ? 4 : !gate_ok ? 5 : g.several_devices ? 6 : (g.kept_given && g.capacity < g.n) ? 7 : 0;
      const GateVerdict v = plan_gate(g);
      ++gate_checks;
      if (v.rule != want || (want == 0) != (v.status == VGICP_OK) || (want != 0 && (v.status != VGICP_ERR_BAD_ARGUMENT || !v.text)) ||
          gate_in_range(gate) != gate_ok) {
        std::printf("MISMATCH (gate): gate %g bits %u -> rule %d, expected %d\n", gate, bits, v.rule, want);
        return 1;
      }
    }
  std::printf("ok %llu verdicts (%llu refused, %llu nothing to do), %llu gate checks\n", checks, refused, nothing, gate_checks);
  return 0;
}
