// CPU check of what vgicp_map_merge decides before it touches the device (eskf_lio_amd/csrc/vgicp_merge_plan.h): its
// refusals in the order of include/vgicp_hip_map_merge.h, over every combination of its facts — the first rule that
// applies is the one reported — the growth it plans for (the insertion's) and the layout of its scratch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "vgicp_merge_plan.h"

using namespace vgicp;

int main() {
  unsigned long long checks = 0, by_rule[14] = {0};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double radii[] = {0.0, 2.5, inf, -0.0, -1.0, -inf, nan};
  const uint64_t voxels[] = {0, 1, 2000, 0xFFFFFFFFull, 0x100000000ull};
  // dst tables: {slots, voxels, tombstones}
  const uint64_t tables[][3] = {{1024, 0, 0}, {1024, 100, 400}, {1ull << 32, 1ull << 30, 0}, {1ull << 32, 1ull << 31, 0}};
  for (uint32_t bits = 0; bits < (1u << 15); ++bits)
    for (const double radius : radii)
      for (const uint64_t v : voxels)
        for (const auto& t : tables) for (int same_size = 0; same_size < 2; ++same_size) {
          MergeFacts f;
          f.dst = bits & 1u;
          f.src = (bits >> 1) & 1u;
          f.params = (bits >> 2) & 1u;
          f.dst_build = (bits >> 3) & 1u;
          f.src_build = (bits >> 4) & 1u;
          f.several_devices = (bits >> 5) & 1u;
          f.same_context = (bits >> 6) & 1u;
          f.same_device = (bits >> 7) & 1u;
          f.reserved = (bits >> 8) & 1u ? 0 : 1ull << 40;
          f.center_finite = (bits >> 9) & 1u;
          f.frame_finite = (bits >> 10) & 1u;
          f.dst_has_map = (bits >> 11) & 1u;
          f.src_has_map = (bits >> 12) & 1u;
          f.dst_raw = (bits >> 13) & 1u;
          f.settled = (bits >> 14) & 1u;
          // the two sizes: equal, or apart in the last bit
          const double h = 0.5, h1 = std::nextafter(0.5, 1.0);
          std::memcpy(&f.dst_voxel_bits, &h, 8);
          std::memcpy(&f.src_voxel_bits, same_size ? &h : &h1, 8);
          f.radius = radius;
          f.src_voxels = v;
          f.dst_slots = t[0];
          f.dst_voxels = t[1];
          f.dst_tombstones = t[2];
          // the insertion's growth rule, restated: load (FULL + TOMB + incoming) <= 1/2, a new table for load <= 1/4
          const uint64_t used = t[1] + t[2] + v;
          uint64_t grown = 0;
          if (used * 2 > t[0]) {
            grown = kMinSlots;
            while (grown < (t[1] + v) * 4) grown <<= 1;
          }
          int want = 0;
          if (!f.dst || !f.src || !f.params) want = 1;
          else if (!f.dst_build || !f.src_build) want = 2;
          else if (f.several_devices) want = 3;
          else if (f.same_context) want = 4;
          else if (!f.same_device) want = 5;
          else if (f.reserved != 0) want = 6;
          else if (!f.center_finite || !f.frame_finite) want = 7;
          else if (std::isnan(radius) || (radius < 0.0)) want = 8;
          else if (!f.dst_has_map || !f.src_has_map) want = 9;
          else if (f.dst_voxel_bits != f.src_voxel_bits) want = 10;
          else if (f.dst_raw) want = 11;
          else if (f.settled && v > 0xFFFFFFFFull) want = 12;
          else if (f.settled && grown > (1ull << 32)) want = 13;
          const int status = want == 0 ? VGICP_OK : want == 9 ? VGICP_ERR_NOT_READY : VGICP_ERR_BAD_ARGUMENT;
          const MergeVerdict got = plan_merge(f);
          ++checks;
          ++by_rule[got.rule >= 0 && got.rule < 14 ? got.rule : 0];
          bool ok = got.rule == want && got.status == status && (want == 0) == (got.text == nullptr);
          const char* word[14] = {"", "NULL pointer", "not from one build", "multi-device contexts, communicators and peer-connected contexts",
                                  "the same context", "different devices", "reserved", "not finite", "radius", "no voxel map",
                                  "voxel sizes of dst and src differ", "keeps raw points", "more voxels than a resident scan", "2^32 slots"};
          if (ok && want != 0) ok = std::strstr(got.text, word[want]) != nullptr;
          // the entry point's own library asks rules 1 and 2 and nothing else
          const MergeVerdict hs = plan_merge_handshake(f);
          ok = ok && hs.rule == (want == 1 || want == 2 ? want : 0);
          // a call that passes grows dst's table exactly as an insertion of src_voxels points would
          if (ok && want == 0 && f.settled) {
            const TableGrowth g = plan_merge_growth(f);
            ok = g.grow == (grown != 0) && (!g.grow || g.slots == grown) && !g.too_large;
          }
          if (!ok) {
            std::printf("MISMATCH: bits %u radius %g voxels %llu slots %llu -> rule %d status %d, expected rule %d status %d\n", bits, radius,
                        (unsigned long long)v, (unsigned long long)t[0], got.rule, got.status, want, status);
            return 1;
          }
        }
  // the scratch: every piece at a 256-byte boundary, in order, none overlapping the next, a line per contributor, the
  // sort's splitters as vgicp_sort.h sizes them (2 * align256((n / 4 + 64) * 4))
  for (uint64_t slots : {1024ull, 4096ull, 2097152ull, 1ull << 32})
    for (uint64_t upper : {0ull, 1ull, 255ull, 2000ull, 1000000ull, 0xFFFFFFFFull}) {
      const MergeWork w = merge_work(slots, upper);
      const uint64_t m = upper ? upper : 1;
      const uint64_t at[9] = {w.submap_at, w.totals_at, w.moved_at, w.slot_in_at, w.slot_out_at, w.idx_in_at, w.idx_out_at, w.split_at, w.total};
      const uint64_t need[8] = {submap_work_bytes(slots), kMergeTotalWords * 8, m * 128, m * 4, m * 4, m * 4, m * 4,
                                2 * (((m / 4 + 64) * 4 + 255) & ~255ull)};
      ++checks;
      bool ok = w.submap_at == 0 && sizeof(MergeMoved) == 128 && alignof(MergeMoved) == 128;
      for (int k = 0; k < 8 && ok; ++k) ok = at[k] % 256 == 0 && at[k] + need[k] <= at[k + 1];
      if (!ok) {
        std::printf("MISMATCH: merge_work(%llu, %llu)\n", (unsigned long long)slots, (unsigned long long)upper);
        return 1;
      }
    }
  std::printf("ok %llu checks:", checks);
  for (int r = 1; r <= 13; ++r) std::printf(" rule %d %llu", r, by_rule[r]);
  std::printf(" passed %llu\n", by_rule[0]);
  return 0;
}
