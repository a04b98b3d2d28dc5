// What a map update decides before it touches the device (eskf_lio_amd/csrc/vgicp_map_plan.h), enumerated on the CPU
// against the predicates the entry points and the grow paths spelled out by hand before they became these functions —
// copied here as they stood: vgicp_map_reset's and raw_reset's first sizes, ensure_table's and ensure_raw's arithmetic,
// insertion_lists_stay_short, and the checks of vgicp_map_insert_scan, vgicp_map_insert_resident,
// vgicp_map_insert_resident_async and vgicp_internal::map_insert_device, each in its own order.  The grids sit exactly on
// and one past every boundary; nothing is skipped, and every outcome has to turn up.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "vgicp_map_plan.h"

using namespace vgicp;

namespace old {
constexpr uint64_t kMinSlots = 1024, kRawMinEntries = 4096, kRawMaxEntries = 1ull << 31;
uint64_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}
template <class T> T max_of(T a, T b) { return a > b ? a : b; }
template <class T> T min_of(T a, T b) { return a < b ? a : b; }

// vgicp_map_reset + alloc_table
struct Table { bool grow; uint64_t slots; bool too_large; };
Table map_reset(size_t capacity_hint) {
  const uint64_t slots = next_pow2(max_of<uint64_t>(kMinSlots, (uint64_t)capacity_hint * 4));
  return {true, slots, slots > (1ull << 32)};
}
// raw_reset
uint64_t raw_reset(size_t raw_hint) {
  return min_of(kRawMaxEntries, next_pow2(max_of<uint64_t>(kRawMinEntries, (uint64_t)raw_hint * 4)));
}
// ensure_table + alloc_table
Table ensure_table(bool table, uint64_t ctx_slots, uint64_t voxels, uint64_t tombstones, uint64_t insert_pending_upper,
                   uint64_t incoming) {
  const uint64_t used = voxels + tombstones + incoming + insert_pending_upper;
  if (table && used * 2 <= ctx_slots) return {false, 0, false};
  const uint64_t slots = next_pow2(max_of<uint64_t>(kMinSlots, (voxels + incoming) * 4));
  return {true, slots, slots > (1ull << 32)};
}
// ensure_raw
bool raw_returns_early(uint64_t raw_used_upper, uint64_t n, uint64_t raw_capacity) { return raw_used_upper + n <= raw_capacity; }
struct Raw { uint64_t cap; bool too_large; };
Raw ensure_raw(uint64_t live, uint64_t n, uint64_t raw_capacity) {
  uint64_t cap = raw_capacity;
  while (cap < kRawMaxEntries && 2 * (live + n) > cap) cap *= 2;
  return {cap, live + n > cap};
}
bool insertion_lists_stay_short(double voxel_size, double prep_voxel, bool insert_sort) {
  if (!(prep_voxel > 0.0) || insert_sort) return false;
  const double per_axis = std::ceil(voxel_size / prep_voxel) + 1.0;
  return per_axis * per_axis * per_axis <= 64.0;
}

// the four insertion entries: what they return before they touch the device.  text nullptr: not refused
struct Ctx { bool table, scan_ready, raw_on, shard_only; };
struct Verdict { int status; const char* text; bool nothing; };
const Verdict kGo{VGICP_OK, nullptr, false}, kNothing{VGICP_OK, nullptr, true};
Verdict fail(int status, const char* text) { return {status, text, false}; }

Verdict map_insert_scan(const Ctx* ctx, size_t n, bool pointers, uint64_t max_points_per_voxel) {
  if (!ctx->table) return fail(VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (n == 0) return kNothing;
  if (!pointers) return fail(VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  if (max_points_per_voxel == 0) return fail(VGICP_ERR_BAD_ARGUMENT, "max_points_per_voxel must be >= 1");
  if (ctx->raw_on && max_points_per_voxel > 0xFFFFFFFFull)
    return fail(VGICP_ERR_BAD_ARGUMENT, "max_points_per_voxel must be < 2^32 while the map keeps raw points");
  if (n > 0x7FFFFFFFull) return fail(VGICP_ERR_BAD_ARGUMENT, "scan too large");
  return kGo;
}
// vgicp_map_insert_resident and vgicp_map_insert_resident_async: the same checks in the same order (they differ in when
// they settle: before all of it, or between the shard refusal and n == 0)
Verdict map_insert_resident(const Ctx* ctx, size_t ctx_n, bool transform, uint64_t max_points_per_voxel) {
  if (!ctx->table) return fail(VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (!ctx->scan_ready) return fail(VGICP_ERR_NOT_READY, "no scan resident: call vgicp_scan_upload first");
  if (!transform) return fail(VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  if (max_points_per_voxel == 0) return fail(VGICP_ERR_BAD_ARGUMENT, "max_points_per_voxel must be >= 1");
  if (ctx->raw_on && max_points_per_voxel > 0xFFFFFFFFull)
    return fail(VGICP_ERR_BAD_ARGUMENT, "max_points_per_voxel must be < 2^32 while the map keeps raw points");
  if (ctx->shard_only) return fail(VGICP_ERR_BAD_ARGUMENT, "resident scan is a shard: use vgicp_map_insert_scan with the whole scan");
  const size_t n = ctx_n;
  if (n == 0) return kNothing;
  return kGo;
}
Verdict map_insert_device(const Ctx* ctx, size_t n, bool transform, uint64_t max_points_per_voxel) {
  if (!ctx->table) return fail(VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first");
  if (!transform) return fail(VGICP_ERR_BAD_ARGUMENT, "NULL pointer");
  if (max_points_per_voxel == 0) return fail(VGICP_ERR_BAD_ARGUMENT, "max_points_per_voxel must be >= 1");
  if (ctx->raw_on && max_points_per_voxel > 0xFFFFFFFFull)
    return fail(VGICP_ERR_BAD_ARGUMENT, "max_points_per_voxel must be < 2^32 while the map keeps raw points");
  if (n > 0x7FFFFFFFull) return fail(VGICP_ERR_BAD_ARGUMENT, "scan too large");
  if (n == 0) return kNothing;
  return kGo;
}
}  // namespace old

static unsigned long long visited = 0;
// every outcome, counted as the PLAN produced it
enum Outcome {
  kTableKept, kTableGrown, kTableTooLarge, kRawFits, kRawCompacted, kRawSameSize, kRawGrown, kRawTooLarge, kShort, kSorted,
  kInsert, kNothingToDo, kNoMap, kNoScan, kNullPointer, kCapZero, kCapRaw, kShard, kScanTooLarge, kOutcomes
};
static const char* const kOutcomeName[kOutcomes] = {
  "table-kept", "table-grown", "table-too-large", "raw-fits", "raw-compacted", "raw-same-size", "raw-grown", "raw-too-large",
  "short-lists", "sorted", "insert", "nothing-to-do", "no-map", "no-scan", "null-pointer", "cap-zero", "cap-raw", "shard",
  "scan-too-large"};
static unsigned long long seen[kOutcomes];

static bool same_table(const TableGrowth& p, const old::Table& o) {
  ++visited;
  ++seen[!p.grow ? kTableKept : p.too_large ? kTableTooLarge : kTableGrown];
  return p.grow == o.grow && p.too_large == o.too_large && (!p.grow || p.slots == o.slots);
}

static int check_first_sizes() {
  const uint64_t one = 1;
  // 4 x hint on and one past the smallest table (1024) and log (4096), 2^32 slots and 2^31 entries
  const uint64_t hints[] = {0, 1, 256, 257, 1024, 1025, one << 29, (one << 29) + 1, one << 30, (one << 30) + 1};
  for (uint64_t hint : hints) {
    if (!same_table(plan_first_table(hint), old::map_reset((size_t)hint)) || plan_first_raw_log(hint) != old::raw_reset((size_t)hint)) {
      std::printf("MISMATCH (first sizes): hint %llu\n", (unsigned long long)hint);
      return 1;
    }
  }
  return 0;
}

static int check_table_growth() {
  const uint64_t one = 1;
  const uint64_t slot_counts[] = {0 /* no table */, 1024, one << 20, one << 32};
  for (uint64_t slots : slot_counts) {
    const bool table = slots != 0;
    // the load exactly at 1/2 and one past, carried by each of the four terms in turn; then (voxels + incoming) x 4 at
    // 2^32 and one past, carried by each of its two terms
    const uint64_t loads[] = {slots / 2, slots / 2 + 1, one << 30, (one << 30) + 1};
    for (int l = 0; l < 4; ++l)
      for (int carrier = 0; carrier < (l < 2 ? 4 : 2); ++carrier) {
        uint64_t term[4] = {0, 0, 0, 0};   // voxels, incoming, tombstones, pending
        term[carrier] = loads[l];
        const TableGrowth p = plan_table_growth(table, slots, term[0], term[2], term[3], term[1]);
        if (!same_table(p, old::ensure_table(table, slots, term[0], term[2], term[3], term[1]))) {
          std::printf("MISMATCH (table growth): slots %llu voxels %llu incoming %llu tombstones %llu pending %llu -> grow %d slots %llu too_large %d\n",
                      (unsigned long long)slots, (unsigned long long)term[0], (unsigned long long)term[1], (unsigned long long)term[2],
                      (unsigned long long)term[3], p.grow, (unsigned long long)p.slots, p.too_large);
          return 1;
        }
      }
  }
  return 0;
}

static int check_raw_log() {
  const uint64_t one = 1;
  const uint64_t capacities[] = {4096, one << 20, one << 31};
  for (uint64_t cap : capacities) {
    // growth: 2 (live + n) at the capacity and one point past, live + n at 2^31 and one past; as one more point on top
    // of the live ones, and as all of them incoming
    const uint64_t totals[] = {cap / 2, cap / 2 + 1, one << 31, (one << 31) + 1};
    for (uint64_t total : totals)
      for (int split = 0; split < 2; ++split) {
        const uint64_t n = split ? total : 1, live = total - n;
        const RawGrowth p = plan_raw_growth(live, n, cap);
        const old::Raw o = old::ensure_raw(live, n, cap);
        ++visited;
        ++seen[p.too_large ? kRawTooLarge : p.capacity == cap ? kRawSameSize : kRawGrown];
        if (p.capacity != o.cap || p.too_large != o.too_large) {
          std::printf("MISMATCH (raw growth): capacity %llu live %llu n %llu -> %llu too_large %d\n", (unsigned long long)cap,
                      (unsigned long long)live, (unsigned long long)n, (unsigned long long)p.capacity, p.too_large);
          return 1;
        }
      }
    // compaction: used + n at the capacity and one past
    for (uint64_t total : {cap, cap + 1})
      for (int split = 0; split < 2; ++split) {
        const uint64_t n = split ? total : 1, used = total - n;
        const bool compaction = raw_log_needs_compaction(used, n, cap);
        ++visited;
        ++seen[compaction ? kRawCompacted : kRawFits];
        if (compaction == old::raw_returns_early(used, n, cap)) {
          std::printf("MISMATCH (raw compaction): capacity %llu used %llu n %llu -> %d\n", (unsigned long long)cap,
                      (unsigned long long)used, (unsigned long long)n, compaction);
          return 1;
        }
      }
  }
  return 0;
}

static int check_short_lists() {
  struct Pair { double map_voxel, scan_voxel; };
  Pair pairs[13];
  int count = 0;
  for (double scan_voxel : {0.25, 1.0}) {   // exact in binary: map voxel / scan voxel is the ratio meant
    for (double ratio : {1.0, 2.0, 3.0, 4.0}) pairs[count++] = {ratio * scan_voxel, scan_voxel};
    pairs[count++] = {std::nextafter(3.0 * scan_voxel, 4.0), scan_voxel};   // 3 + one ulp: ceil() gives 4, 125 lists
  }
  for (double scan_voxel : {0.0, -0.3, std::numeric_limits<double>::quiet_NaN()}) pairs[count++] = {0.3, scan_voxel};
  for (int i = 0; i < count; ++i)
    for (int insert_sort = 0; insert_sort < 2; ++insert_sort) {
      const bool p = insertion_lists_stay_short(pairs[i].map_voxel, pairs[i].scan_voxel, insert_sort != 0);
      ++visited;
      ++seen[p ? kShort : kSorted];
      if (p != old::insertion_lists_stay_short(pairs[i].map_voxel, pairs[i].scan_voxel, insert_sort != 0)) {
        std::printf("MISMATCH (short lists): map voxel %.17g scan voxel %.17g insert_sort %d -> %d\n", pairs[i].map_voxel,
                    pairs[i].scan_voxel, insert_sort, p);
        return 1;
      }
    }
  return 0;
}

static Outcome outcome_of(const InsertVerdict& v) {
  if (v.status == VGICP_OK) return v.nothing_to_do ? kNothingToDo : kInsert;
  const char* const texts[] = {"no voxel map", "no scan resident", "NULL pointer", "max_points_per_voxel must be >= 1",
                               "max_points_per_voxel must be < 2^32", "resident scan is a shard", "scan too large"};
  for (int i = 0; i < 7; ++i)
    if (std::strncmp(v.text, texts[i], std::strlen(texts[i])) == 0) return (Outcome)(kNoMap + i);
  return kOutcomes;
}

static int check_insert_verdict() {
  const uint64_t one = 1;
  const InsertEntry entries[] = {InsertEntry::Scan, InsertEntry::Resident, InsertEntry::ResidentAsync, InsertEntry::Device};
  const uint64_t ns[] = {0, 1, (one << 31) - 1, one << 31};
  const uint64_t caps[] = {0, 1, (one << 32) - 1, one << 32};
  for (InsertEntry entry : entries)
    for (uint32_t bits = 0; bits < 32; ++bits)
      for (uint64_t n : ns)
        for (uint64_t cap : caps) {
          InsertFacts f;
          f.entry = entry;
          f.has_table = bits & 1u;
          f.scan_resident = (bits >> 1) & 1u;
          f.pointers = (bits >> 2) & 1u;
          f.raw_on = (bits >> 3) & 1u;
          f.shard_only = (bits >> 4) & 1u;
          f.n = n;
          f.points_per_voxel = cap;
          const old::Ctx ctx{f.has_table, f.scan_resident, f.raw_on, f.shard_only};
          const old::Verdict o = entry == InsertEntry::Scan ? old::map_insert_scan(&ctx, (size_t)n, f.pointers, cap)
                               : entry == InsertEntry::Device ? old::map_insert_device(&ctx, (size_t)n, f.pointers, cap)
                                                              : old::map_insert_resident(&ctx, (size_t)n, f.pointers, cap);
          const InsertVerdict p = plan_insert(f);
          ++visited;
          const Outcome out = outcome_of(p);
          if (out != kOutcomes) ++seen[out];
          const bool same_text = (p.text == nullptr) == (o.text == nullptr) && (!p.text || std::strcmp(p.text, o.text) == 0);
          if (out == kOutcomes || p.status != o.status || !same_text || p.nothing_to_do != o.nothing) {
            std::printf("MISMATCH (insert verdict): entry %d table %d scan %d pointers %d raw %d shard %d n %llu cap %llu -> %d '%s' nothing %d, "
                        "was %d '%s' nothing %d\n", (int)entry, f.has_table, f.scan_resident, f.pointers, f.raw_on, f.shard_only,
                        (unsigned long long)n, (unsigned long long)cap, p.status, p.text ? p.text : "", p.nothing_to_do, o.status,
                        o.text ? o.text : "", o.nothing);
            return 1;
          }
        }
  return 0;
}

int main() {
  if (check_first_sizes() || check_table_growth() || check_raw_log() || check_short_lists() || check_insert_verdict()) return 1;
  std::printf("ok %llu checks:", visited);
  for (int i = 0; i < kOutcomes; ++i) std::printf(" %s %llu", kOutcomeName[i], seen[i]);
  std::printf("\n");
  return 0;
}
