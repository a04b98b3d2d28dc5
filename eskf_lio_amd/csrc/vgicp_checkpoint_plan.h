// vgicp_checkpoint_plan.h — what the map checkpoint (include/vgicp_hip_map_checkpoint.h) decides on the host: the blob's
// layout, its checksum, THE CHECK a blob has to pass before a restore touches anything, and the geometry of the
// launches.  Pure functions of plain bytes and facts (no HIP call, no context), so that a CPU program can enumerate them
// (tests/native/checkpoint_plan.cpp).  Every multi-byte field is read and written with memcpy: a blob may lie at any
// address.  Little-endian hosts only, as the module.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/vgicp_hip_map_checkpoint.h"
#include "vgicp_map_plan.h"
#include "vgicp_submap_plan.h"

namespace vgicp {

constexpr uint64_t kCheckpointHeader = VGICP_CHECKPOINT_HEADER_BYTES, kCheckpointRecord = VGICP_CHECKPOINT_RECORD_BYTES;
constexpr char kCheckpointMagic[9] = "VGICPMAP";
constexpr int32_t kCheckpointStateFull = 1;   // SLOT_FULL (vgicp_device.h, which a CPU program cannot include)
// byte offsets inside a record: the state, the count, the spare word
constexpr uint64_t kRecordStateAt = 12, kRecordCountAt = 112, kRecordSpareAt = 120;

struct CheckpointHeader {   // the header's fields as the blob holds them
  uint32_t format = VGICP_CHECKPOINT_FORMAT, header_bytes = VGICP_CHECKPOINT_HEADER_BYTES;
  uint64_t total_bytes = 0;
  double voxel_size = 0.0;
  uint64_t slots = 0, voxels = 0, tombstones = 0, raw_points = 0;
  uint32_t flags = 0, record_bytes = VGICP_CHECKPOINT_RECORD_BYTES;
  uint64_t checksum = 0;
};

inline uint64_t pad8(uint64_t v) { return (v + 7) & ~7ull; }
// where the sections lie, from the blob's first byte
struct CheckpointLayout {
  uint64_t full_at = 0, tomb_at = 0, records_at = 0, raw_at = 0, total = 0;
};
inline CheckpointLayout checkpoint_layout(uint64_t voxels, uint64_t tombstones, uint64_t raw_points) {
  CheckpointLayout l;
  l.full_at = kCheckpointHeader;
  l.tomb_at = l.full_at + pad8(4 * voxels);
  l.records_at = l.tomb_at + pad8(4 * tombstones);
  l.raw_at = l.records_at + kCheckpointRecord * voxels;
  l.total = l.raw_at + 24 * raw_points;
  return l;
}

// THE checksum loop, written once: word i of src (as u64) times 2 i + 1, summed mod 2^64; bytes: a multiple of 8.
// COPY: the words are also written to dst on the way, so that one pass reads, sums and writes.
template <bool COPY> inline uint64_t checkpoint_sum_words(void* dst, const void* src, uint64_t bytes) {
  const unsigned char* s = static_cast<const unsigned char*>(src);
  unsigned char* d = static_cast<unsigned char*>(dst);
  const uint64_t words = bytes / 8;
  uint64_t sum[4] = {0, 0, 0, 0};   // four chains: the adds of one do not wait for the other's
  uint64_t i = 0;
  for (; i + 4 <= words; i += 4) {
    uint64_t w[4];
    std::memcpy(w, s + 8 * i, 32);
    if (COPY) std::memcpy(d + 8 * i, w, 32);
    for (int k = 0; k < 4; ++k) sum[k] += w[k] * (2 * (i + k) + 1);
  }
  for (; i < words; ++i) {
    uint64_t w;
    std::memcpy(&w, s + 8 * i, 8);
    if (COPY) std::memcpy(d + 8 * i, &w, 8);
    sum[0] += w * (2 * i + 1);
  }
  return (sum[0] + sum[1]) + (sum[2] + sum[3]);
}
inline uint64_t checkpoint_checksum(const void* payload, uint64_t bytes) { return checkpoint_sum_words<false>(nullptr, payload, bytes); }
inline uint64_t checkpoint_copy_checksum(void* dst, const void* src, uint64_t bytes) { return checkpoint_sum_words<true>(dst, src, bytes); }

template <class T> inline T checkpoint_load(const void* at) {
  T v;
  std::memcpy(&v, at, sizeof v);
  return v;
}
inline void checkpoint_write_header(void* out, const CheckpointHeader& h) {
  unsigned char* b = static_cast<unsigned char*>(out);
  std::memset(b, 0, kCheckpointHeader);
  std::memcpy(b, kCheckpointMagic, 8);
  std::memcpy(b + 8, &h.format, 4);
  std::memcpy(b + 12, &h.header_bytes, 4);
  std::memcpy(b + 16, &h.total_bytes, 8);
  std::memcpy(b + 24, &h.voxel_size, 8);
  std::memcpy(b + 32, &h.slots, 8);
  std::memcpy(b + 40, &h.voxels, 8);
  std::memcpy(b + 48, &h.tombstones, 8);
  std::memcpy(b + 56, &h.raw_points, 8);
  std::memcpy(b + 64, &h.flags, 4);
  std::memcpy(b + 68, &h.record_bytes, 4);
  std::memcpy(b + 72, &h.checksum, 8);
}
inline CheckpointHeader checkpoint_read_header(const void* blob) {   // of at least 128 bytes
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  CheckpointHeader h;
  h.format = checkpoint_load<uint32_t>(b + 8);
  h.header_bytes = checkpoint_load<uint32_t>(b + 12);
  h.total_bytes = checkpoint_load<uint64_t>(b + 16);
  h.voxel_size = checkpoint_load<double>(b + 24);
  h.slots = checkpoint_load<uint64_t>(b + 32);
  h.voxels = checkpoint_load<uint64_t>(b + 40);
  h.tombstones = checkpoint_load<uint64_t>(b + 48);
  h.raw_points = checkpoint_load<uint64_t>(b + 56);
  h.flags = checkpoint_load<uint32_t>(b + 64);
  h.record_bytes = checkpoint_load<uint32_t>(b + 68);
  h.checksum = checkpoint_load<uint64_t>(b + 72);
  return h;
}

// THE CHECK: 0 when the blob passes, else the number of the first rule of the header's list that it fails.  *out: the
// header's fields (as far as rule 1 lets them be read; else untouched).
inline int checkpoint_check(const void* blob, uint64_t bytes, CheckpointHeader* out = nullptr) {
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  if (!b || bytes < kCheckpointHeader || std::memcmp(b, kCheckpointMagic, 8) != 0) return 1;
  const CheckpointHeader h = checkpoint_read_header(b);
  if (out) *out = h;
  if (h.format != VGICP_CHECKPOINT_FORMAT || h.header_bytes != kCheckpointHeader || h.record_bytes != kCheckpointRecord) return 2;
  for (uint64_t i = 80; i < kCheckpointHeader; ++i)
    if (b[i] != 0) return 3;
  if ((h.flags & ~VGICP_CHECKPOINT_RAW_POINTS) != 0) return 3;
  if (!std::isfinite(h.voxel_size) || !(h.voxel_size > 0.0)) return 4;
  if (h.slots < kMinSlots || h.slots > kMaxSlots || (h.slots & (h.slots - 1)) != 0) return 5;
  if (h.voxels > h.slots || h.tombstones > h.slots || 2 * (h.voxels + h.tombstones) > h.slots) return 6;
  const bool raw = (h.flags & VGICP_CHECKPOINT_RAW_POINTS) != 0;
  if ((!raw && h.raw_points != 0) || h.raw_points > kRawMaxEntries) return 7;
  const CheckpointLayout l = checkpoint_layout(h.voxels, h.tombstones, h.raw_points);   // no overflow: rules 5 - 7 bound F, T, P
  if (bytes != h.total_bytes || h.total_bytes != l.total) return 8;
  if (checkpoint_checksum(b + kCheckpointHeader, l.total - kCheckpointHeader) != h.checksum) return 9;
  const unsigned char *full = b + l.full_at, *tomb = b + l.tomb_at, *records = b + l.records_at;
  for (uint64_t j = 0; j < h.voxels; ++j) {
    const uint32_t s = checkpoint_load<uint32_t>(full + 4 * j);
    if (s >= h.slots || (j > 0 && s <= checkpoint_load<uint32_t>(full + 4 * (j - 1)))) return 10;
  }
  for (uint64_t j = 0; j < h.tombstones; ++j) {
    const uint32_t s = checkpoint_load<uint32_t>(tomb + 4 * j);
    if (s >= h.slots || (j > 0 && s <= checkpoint_load<uint32_t>(tomb + 4 * (j - 1)))) return 11;
  }
  for (uint64_t i = 0, j = 0; i < h.voxels && j < h.tombstones;) {   // both ascend: one merge pass
    const uint32_t f = checkpoint_load<uint32_t>(full + 4 * i), t = checkpoint_load<uint32_t>(tomb + 4 * j);
    if (f == t) return 12;
    if (f < t) ++i; else ++j;
  }
  uint64_t points = 0;
  bool sum_fits = true;
  for (uint64_t j = 0; j < h.voxels; ++j) {
    const unsigned char* r = records + kCheckpointRecord * j;
    const uint64_t count = checkpoint_load<uint64_t>(r + kRecordCountAt);
    if (checkpoint_load<int32_t>(r + kRecordStateAt) != kCheckpointStateFull || checkpoint_load<uint64_t>(r + kRecordSpareAt) != 0 || count < 1)
      return 13;
    if (sum_fits && count <= h.raw_points - points) points += count;   // points <= P throughout: no overflow
    else sum_fits = false;
  }
  if (raw && (!sum_fits || points != h.raw_points)) return 14;
  return 0;
}
inline const char* checkpoint_rule_text(int rule) {
  static const char* const text[VGICP_CHECKPOINT_RULES + 1] = {
      "the blob passes",
      "rule 1: fewer than 128 bytes, or the magic is not VGICPMAP",
      "rule 2: format, header_bytes or record_bytes is not format 1's",
      "rule 3: a reserved byte is not zero, or an unknown flag is set",
      "rule 4: voxel_size is not finite and > 0",
      "rule 5: slots is not a power of two within 1024 .. 2^32",
      "rule 6: 2 (voxels + tombstones) exceeds slots",
      "rule 7: raw_points without the raw-points flag, or beyond 2^31",
      "rule 8: bytes, total_bytes and the formula disagree",
      "rule 9: the checksum does not match",
      "rule 10: full_slots is not strictly ascending below slots",
      "rule 11: tomb_slots is not strictly ascending below slots",
      "rule 12: a slot is in both lists",
      "rule 13: a record is not FULL, its spare word is not 0 or its count is 0",
      "rule 14: the records' counts do not sum to raw_points"};
  return rule >= 0 && rule <= VGICP_CHECKPOINT_RULES ? text[rule] : "unknown rule";
}

// ---- what the two calls refuse before the check (the header's lists) ----
struct CheckpointFacts {
  bool pointers = true;          // every required pointer is there
  bool same_build = true;
  bool several_devices = false;
  bool has_map = true;           // checkpoint only
};
using CheckpointVerdict = ResidentVerdict;
inline CheckpointVerdict plan_checkpoint_handshake(const CheckpointFacts& f) {
  if (!f.pointers) return {1, VGICP_ERR_BAD_ARGUMENT, "NULL pointer"};
  if (!f.same_build) return {2, VGICP_ERR_BAD_ARGUMENT, "context and libvgicp_hip_map_checkpoint.so are not from one build of the module"};
  return {};
}
inline CheckpointVerdict plan_checkpoint(const CheckpointFacts& f, bool restore) {
  const CheckpointVerdict first = plan_checkpoint_handshake(f);
  if (first.rule != 0) return first;
  if (f.several_devices)
    return {3, VGICP_ERR_BAD_ARGUMENT, "the map checkpoint works on a single-device context: not on multi-device contexts, "
                                       "communicators and peer-connected contexts"};
  if (!restore && !f.has_map) return {4, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first"};
  return {};
}

// ---- the launches.  MARK and EMIT walk the table in the submap's groups (vgicp_submap_plan.h): kSubmapGroupSlots slots
// per workgroup, kSubmapGroupWords ballot words per group and kind.  The call's scratch, each piece at a 256-byte
// boundary: [groups][2][words] ballots (FULL, TOMB), [groups][words] the FULL counts' sums per ballot word,
// [3][groups] the groups' counts (FULL, TOMB, raw), 4 totals, and with raw points one offset per slot ----
inline uint64_t checkpoint_align256(uint64_t v) { return (v + 255) & ~255ull; }
struct CheckpointWork {
  uint64_t ballots_at = 0, word_raw_at = 0, counts_at = 0, totals_at = 0, offsets_at = 0;
  uint64_t full_at = 0, tomb_at = 0, records_at = 0, raw_at = 0;   // the sections, each aligned for 16-byte accesses
  uint64_t total = 0;
};
inline CheckpointWork checkpoint_work(uint64_t slots, uint64_t voxels, uint64_t tombstones, bool raw, uint64_t raw_room) {
  const uint64_t g = submap_groups(slots);
  CheckpointWork w;
  uint64_t at = 0;
  const auto take = [&at](uint64_t bytes) { const uint64_t here = at; at += checkpoint_align256(bytes); return here; };
  w.ballots_at = take(g * 2 * kSubmapGroupWords * 8);
  w.word_raw_at = take(g * kSubmapGroupWords * 4);
  w.counts_at = take(3 * g * 4);
  w.totals_at = take(4 * 8);
  w.offsets_at = take(raw ? slots * 4 : 0);
  w.full_at = take(4 * voxels);
  w.tomb_at = take(4 * tombstones);
  w.records_at = take(kCheckpointRecord * voxels);
  w.raw_at = take(raw ? 24 * raw_room : 0);
  w.total = at;
  return w;
}
// the restore's: the sections, then (raw points) the sums of the counts per block of kRestoreBlock records and a total
constexpr uint32_t kRestoreBlock = 1024;
inline uint32_t restore_blocks(uint64_t voxels) { return (uint32_t)((voxels + kRestoreBlock - 1) / kRestoreBlock); }
struct RestoreWork {
  uint64_t full_at = 0, tomb_at = 0, records_at = 0, raw_at = 0, sums_at = 0, totals_at = 0, total = 0;
};
inline RestoreWork restore_work(uint64_t voxels, uint64_t tombstones, uint64_t raw_points) {
  RestoreWork w;
  uint64_t at = 0;
  const auto take = [&at](uint64_t bytes) { const uint64_t here = at; at += checkpoint_align256(bytes); return here; };
  w.full_at = take(4 * voxels);
  w.tomb_at = take(4 * tombstones);
  w.records_at = take(kCheckpointRecord * voxels);
  w.raw_at = take(24 * raw_points);
  w.sums_at = take(4ull * restore_blocks(voxels));
  w.totals_at = take(4 * 8);
  w.total = at;
  return w;
}
// the raw log a restore makes: twice what it holds, as a growth leaves it (plan_raw_growth)
inline uint64_t restore_raw_capacity(uint64_t raw_points) {
  return std::min(kRawMaxEntries, next_pow2(std::max<uint64_t>(kRawMinEntries, 2 * raw_points)));
}

}  // namespace vgicp
