// CPU check of what vgicp_locate_resident decides before it touches the device (eskf_lio_amd/csrc/vgicp_locate_plan.h):
// its refusals in the order of include/vgicp_hip_map_locate.h, over every combination of its facts — the first rule that
// applies is the one reported — and the geometry of its score launch.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "vgicp_locate_plan.h"

using namespace vgicp;

int main() {
  unsigned long long checks = 0, by_rule[7] = {0};
  const uint64_t ks[] = {0, 1, 64, 65};
  const int64_t levels[] = {-1, 0, 2, 4, 5};
  const int64_t windows[][3] = {{0, 0, 0}, {4, 4, 1}, {32, 0, 0}, {33, 0, 0}, {0, -1, 0}, {10, 10, 4}, {10, 10, 5}, {32, 32, 32}};
  const uint64_t strides[] = {0, 1, 4};
  for (uint32_t bits = 0; bits < 128; ++bits)
    for (const uint64_t k : ks)
      for (const int64_t level : levels)
        for (const auto& w : windows)
          for (const uint64_t stride : strides)
            for (int requested = 0; requested <= VGICP_LEVELS_MAX; requested += 2) {
              LocateFacts f;
              f.ctx = bits & 1u;
              f.pointers = (bits >> 1) & 1u;
              f.poses_finite = (bits >> 2) & 1u;
              f.at.several_devices = (bits >> 3) & 1u;
              f.at.has_map = (bits >> 4) & 1u;
              f.at.scan_resident = (bits >> 5) & 1u;
              f.at.settled = (bits >> 6) & 1u;
              f.k = k;
              f.level = level;
              for (int a = 0; a < 3; ++a) f.window[a] = w[a];
              f.stride = stride;
              f.requested = requested;
              bool widths = true;
              for (int a = 0; a < 3; ++a) widths = widths && w[a] >= 0 && w[a] <= VGICP_LOCATE_MAX_HALF_WIDTH;
              const bool cells = widths && (2 * w[0] + 1) * (2 * w[1] + 1) * (2 * w[2] + 1) <= VGICP_LOCATE_MAX_CELLS;
              int want = 0;
              if (!f.ctx || !f.pointers) want = 1;
              else if (k < 1 || k > 64 || level < 0 || level > VGICP_LEVELS_MAX || !cells || stride < 1) want = 2;
              else if (level > requested) want = 3;
              else if (!f.poses_finite) want = 4;
              else if (f.at.several_devices) want = 5;
              else if (!f.at.has_map || !f.at.scan_resident) want = 6;
              const int status = want == 0 ? VGICP_OK : (want == 3 || want == 6) ? VGICP_ERR_NOT_READY : VGICP_ERR_BAD_ARGUMENT;
              const LocateVerdict v = plan_locate(f);
              ++checks;
              ++by_rule[v.rule >= 0 && v.rule < 7 ? v.rule : 0];
              bool ok = v.rule == want && v.status == status;
              if (want != 0 && f.ctx) ok = ok && v.text != nullptr;        // a NULL context has nowhere to leave a text
              if (want == 0) ok = ok && v.text == nullptr;
              if (ok && want == 2) {   // within rule 2: k, then the level, then a half-width, then the cells, then the stride
                const char* word = (k < 1 || k > 64) ? "k must be" : (level < 0 || level > VGICP_LEVELS_MAX) ? "level must be"
                                   : !widths ? "half-width" : !cells ? "VGICP_LOCATE_MAX_CELLS" : "stride";
                ok = std::strstr(v.text, word) != nullptr;
              }
              if (ok && want == 3) ok = std::strstr(v.text, "vgicp_map_levels_build") != nullptr;
              if (ok && want == 5) ok = std::strstr(v.text, "multi-device contexts, communicators and peer-connected contexts: the resident scan "
                                                            "of a device is a shard there") != nullptr;
              if (ok && want == 6) ok = std::strstr(v.text, f.at.has_map ? "no scan resident" : "no voxel map") != nullptr;
              if (!ok) {
                std::printf("MISMATCH: bits %u k %llu level %lld window %lld %lld %lld stride %llu requested %d -> rule %d status %d, "
                            "expected rule %d status %d\n", bits, (unsigned long long)k, (long long)level, (long long)w[0], (long long)w[1],
                            (long long)w[2], (unsigned long long)stride, requested, v.rule, v.status, want, status);
                return 1;
              }
            }
  // the points that take part and the chunks of the score launch cover them exactly
  for (uint64_t n : {0ull, 1ull, 63ull, 128ull, 129ull, 6000ull, (1ull << 32) - 1})
    for (uint64_t stride : {1ull, 3ull, 4ull, 6000ull, (1ull << 32) - 1}) {
      const uint64_t p = locate_participants(n, stride);
      ++checks;
      uint64_t count = 0;
      if (n <= 6000) {
        for (uint64_t i = 0; i < n; ++i) count += i % stride == 0;
      } else {
        count = (n - 1) / stride + 1;
      }
      const uint32_t chunks = locate_chunks(p);
      if (p != count || (uint64_t)chunks * kLocateChunk < p || (p > 0 && (uint64_t)(chunks - 1) * kLocateChunk >= p) || (p == 0 && chunks != 0)) {
        std::printf("MISMATCH: locate_participants(%llu, %llu) = %llu in %u chunks\n", (unsigned long long)n,
                    (unsigned long long)stride, (unsigned long long)p, chunks);
        return 1;
      }
    }
  std::printf("ok %llu checks:", checks);
  for (int r = 1; r <= 6; ++r) std::printf(" rule %d %llu", r, by_rule[r]);
  std::printf(" passed %llu\n", by_rule[0]);
  return 0;
}
