// checkpoint_plan.cpp — the map checkpoint's host check (eskf_lio_amd/csrc/vgicp_checkpoint_plan.h, checkpoint_check) fed
// with blobs built here: well-formed ones over F x T x raw, one mutation per rule (the checksum recomputed where the rule
// comes behind the checksum, so that rule and not rule 9 is what fires), every truncation length and every single bit
// flip of one small blob.  Counts what it visited; every rule number has to fire; no mutated blob may pass, except
//   - a record's key, mean or covariance changed with the checksum recomputed: the check does not look at them, and
//   - a flipped bit of the header's voxel_size that leaves it finite and > 0: the checksum covers the payload, bytes
//     [128, total_bytes), and rule 4 is all the header says about voxel_size.  Those flips MUST pass (the exception is
//     exact, not lenient).
// With a file name as argument every blob offered is appended to that file as {u32 bytes, i32 verdict, bytes}, for
// tests/test_map_checkpoint_cpu.py to hold tests/map_checkpoint_reference.py's check() against.
// Prints "ok ..." and returns 0, or prints MISMATCH lines and returns 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "vgicp_checkpoint_plan.h"

using namespace vgicp;
using Blob = std::vector<unsigned char>;

static FILE* g_out = nullptr;
static long g_fired[VGICP_CHECKPOINT_RULES + 1] = {0};
static long g_offered = 0, g_mismatch = 0;

static int offer(const Blob& b, size_t bytes) {
  const int rule = checkpoint_check(b.data(), bytes);
  ++g_offered;
  if (rule >= 0 && rule <= VGICP_CHECKPOINT_RULES) ++g_fired[rule];
  if (g_out) {
    const uint32_t n = (uint32_t)bytes;
    const int32_t r = rule;
    std::fwrite(&n, 4, 1, g_out);
    std::fwrite(&r, 4, 1, g_out);
    std::fwrite(b.data(), 1, bytes, g_out);
  }
  return rule;
}
static void expect(const Blob& b, int want, const char* what) {
  const int got = offer(b, b.size());
  if (got != want) {
    std::printf("MISMATCH %s: rule %d, expected %d\n", what, got, want);
    ++g_mismatch;
  }
}
template <class T> static void put(Blob& b, size_t at, T v) { std::memcpy(b.data() + at, &v, sizeof v); }
template <class T> static T get(const Blob& b, size_t at) { return checkpoint_load<T>(b.data() + at); }
static void refresh(Blob& b) {   // the checksum over the payload as it is now
  put<uint64_t>(b, 72, checkpoint_checksum(b.data() + kCheckpointHeader, b.size() - kCheckpointHeader));
}

// F records at slots 3 j + 1 with counts 1 + j % 3, T tombstones at slots 3 j + 2, in a table of 1 024 slots
static Blob make(uint64_t F, uint64_t T, bool raw) {
  uint64_t P = 0;
  for (uint64_t j = 0; j < F; ++j) P += raw ? 1 + j % 3 : 0;
  const CheckpointLayout l = checkpoint_layout(F, T, P);
  Blob b(l.total, 0);
  for (uint64_t j = 0; j < F; ++j) {
    put<uint32_t>(b, l.full_at + 4 * j, (uint32_t)(3 * j + 1));
    const size_t r = l.records_at + kCheckpointRecord * j;
    put<int32_t>(b, r, (int32_t)j);
    put<int32_t>(b, r + 4, -(int32_t)j);
    put<int32_t>(b, r + 8, 7);
    put<int32_t>(b, r + kRecordStateAt, kCheckpointStateFull);
    for (int k = 0; k < 12; ++k) put<double>(b, r + 16 + 8 * k, 0.25 * (double)j + (double)k);
    put<uint64_t>(b, r + kRecordCountAt, 1 + j % 3);
  }
  for (uint64_t j = 0; j < T; ++j) put<uint32_t>(b, l.tomb_at + 4 * j, (uint32_t)(3 * j + 2));
  for (uint64_t p = 0; p < 3 * P; ++p) put<double>(b, l.raw_at + 8 * p, 0.125 * (double)p);
  CheckpointHeader h;
  h.total_bytes = l.total;
  h.voxel_size = 0.5;
  h.slots = 1024;
  h.voxels = F;
  h.tombstones = T;
  h.raw_points = P;
  h.flags = raw ? VGICP_CHECKPOINT_RAW_POINTS : 0u;
  checkpoint_write_header(b.data(), h);
  refresh(b);
  return b;
}

int main(int argc, char** argv) {
  if (argc > 1) g_out = std::fopen(argv[1], "wb");
  long built = 0, mutations = 0, truncations = 0, flips = 0, harmless = 0;

  // ---- well-formed blobs, and the formula
  const uint64_t Fs[] = {0, 1, 2, 64, 65}, Ts[] = {0, 1, 3};
  for (uint64_t F : Fs)
    for (uint64_t T : Ts)
      for (int raw = 0; raw < 2; ++raw) {
        const Blob b = make(F, T, raw != 0);
        const uint64_t P = get<uint64_t>(b, 56);
        if (b.size() != 128 + pad8(4 * F) + pad8(4 * T) + 128 * F + 24 * P) { std::printf("MISMATCH size\n"); ++g_mismatch; }
        expect(b, 0, "well-formed");
        ++built;
      }

  // ---- the checksum by its definition, word by word, at every length and from an odd address; the copying form too
  {
    const Blob big = make(65, 3, true);
    Blob odd(big.size() + 1), copy(big.size());
    std::memcpy(odd.data() + 1, big.data(), big.size());
    for (size_t n = 0; n + kCheckpointHeader <= big.size(); n += 8) {
      uint64_t want = 0;
      for (size_t i = 0; i < n / 8; ++i) want += get<uint64_t>(big, kCheckpointHeader + 8 * i) * (2 * i + 1);
      std::fill(copy.begin(), copy.end(), (unsigned char)0xEE);
      const bool same = checkpoint_checksum(big.data() + kCheckpointHeader, n) == want &&
                        checkpoint_checksum(odd.data() + 1 + kCheckpointHeader, n) == want &&
                        checkpoint_copy_checksum(copy.data() + 1, odd.data() + 1 + kCheckpointHeader, n) == want &&
                        std::memcmp(copy.data() + 1, big.data() + kCheckpointHeader, n) == 0 && copy[0] == 0xEE &&
                        (1 + n >= copy.size() || copy[1 + n] == 0xEE);
      if (!same) { std::printf("MISMATCH checksum of %zu bytes\n", n); ++g_mismatch; }
    }
  }

  // ---- one mutation per rule
  const Blob base = make(2, 3, true), plain = make(2, 3, false);
  const CheckpointLayout l = checkpoint_layout(2, 3, get<uint64_t>(base, 56));
  const auto mutate = [&](int want, const char* what, const Blob& from, auto change, bool recompute) {
    Blob b = from;
    change(b);
    if (recompute) refresh(b);
    expect(b, want, what);
    ++mutations;
  };
  mutate(1, "magic", base, [](Blob& b) { b[3] ^= 0x20; }, false);
  mutate(1, "127 bytes", base, [](Blob& b) { b.resize(127); }, false);
  mutate(1, "no byte", base, [](Blob& b) { b.clear(); }, false);
  mutate(2, "format", base, [](Blob& b) { put<uint32_t>(b, 8, 2); }, false);
  mutate(2, "header_bytes", base, [](Blob& b) { put<uint32_t>(b, 12, 64); }, false);
  mutate(2, "record_bytes", base, [](Blob& b) { put<uint32_t>(b, 68, 64); }, false);
  mutate(3, "reserved", base, [](Blob& b) { b[80] = 1; }, false);
  mutate(3, "reserved, last", base, [](Blob& b) { b[127] = 0x80; }, false);
  mutate(3, "unknown flag", base, [](Blob& b) { put<uint32_t>(b, 64, 3); }, false);
  mutate(4, "voxel_size 0", base, [](Blob& b) { put<double>(b, 24, 0.0); }, false);
  mutate(4, "voxel_size < 0", base, [](Blob& b) { put<double>(b, 24, -0.5); }, false);
  mutate(4, "voxel_size NaN", base, [](Blob& b) { put<double>(b, 24, std::numeric_limits<double>::quiet_NaN()); }, false);
  mutate(4, "voxel_size inf", base, [](Blob& b) { put<double>(b, 24, std::numeric_limits<double>::infinity()); }, false);
  mutate(5, "slots 1000", base, [](Blob& b) { put<uint64_t>(b, 32, 1000); }, false);
  mutate(5, "slots 512", base, [](Blob& b) { put<uint64_t>(b, 32, 512); }, false);
  mutate(5, "slots 2^33", base, [](Blob& b) { put<uint64_t>(b, 32, 1ull << 33); }, false);
  mutate(5, "slots 0", base, [](Blob& b) { put<uint64_t>(b, 32, 0); }, false);
  mutate(6, "voxels 600", base, [](Blob& b) { put<uint64_t>(b, 40, 600); }, false);
  mutate(6, "tombstones 2^63", base, [](Blob& b) { put<uint64_t>(b, 48, 1ull << 63); }, false);
  mutate(6, "F + T wraps", base, [](Blob& b) { put<uint64_t>(b, 40, ~0ull); put<uint64_t>(b, 48, 3); }, false);
  mutate(7, "raw_points without the flag", plain, [](Blob& b) { put<uint64_t>(b, 56, 5); }, false);
  mutate(7, "raw_points 2^31 + 1", base, [](Blob& b) { put<uint64_t>(b, 56, (1ull << 31) + 1); }, false);
  mutate(8, "total_bytes + 8", base, [](Blob& b) { put<uint64_t>(b, 16, get<uint64_t>(b, 16) + 8); }, false);
  mutate(8, "eight bytes more", base, [](Blob& b) { b.resize(b.size() + 8, 0); }, false);
  mutate(8, "voxels + 1", base, [](Blob& b) { put<uint64_t>(b, 40, 3); }, false);
  mutate(9, "payload bit", base, [&](Blob& b) { b[l.records_at + 20] ^= 1; }, false);
  mutate(9, "checksum bit", base, [](Blob& b) { b[72] ^= 1; }, false);
  mutate(9, "two words swapped", base, [&](Blob& b) {
    for (int k = 0; k < 8; ++k) std::swap(b[l.records_at + 16 + k], b[l.records_at + 24 + k]);
  }, false);
  mutate(10, "full_slots equal", base, [&](Blob& b) { put<uint32_t>(b, l.full_at + 4, get<uint32_t>(b, l.full_at)); }, true);
  mutate(10, "full_slots descending", base, [&](Blob& b) { put<uint32_t>(b, l.full_at, 9); }, true);
  mutate(10, "full slot = slots", base, [&](Blob& b) { put<uint32_t>(b, l.full_at + 4, 1024); }, true);
  mutate(11, "tomb_slots equal", base, [&](Blob& b) { put<uint32_t>(b, l.tomb_at + 4, get<uint32_t>(b, l.tomb_at)); }, true);
  mutate(11, "tomb slot = slots", base, [&](Blob& b) { put<uint32_t>(b, l.tomb_at + 8, 1024); }, true);
  mutate(12, "a slot in both lists", base, [&](Blob& b) { put<uint32_t>(b, l.tomb_at, get<uint32_t>(b, l.full_at)); }, true);
  mutate(12, "the last slot in both lists", base, [&](Blob& b) { put<uint32_t>(b, l.tomb_at + 4, get<uint32_t>(b, l.full_at + 4)); }, true);
  mutate(13, "state TOMB", base, [&](Blob& b) { put<int32_t>(b, l.records_at + kRecordStateAt, 2); }, true);
  mutate(13, "spare word", base, [&](Blob& b) { put<uint64_t>(b, l.records_at + kCheckpointRecord + kRecordSpareAt, 1ull << 40); }, true);
  mutate(13, "count 0", base, [&](Blob& b) { put<uint64_t>(b, l.records_at + kRecordCountAt, 0); }, true);
  mutate(14, "a count one more", base, [&](Blob& b) { put<uint64_t>(b, l.records_at + kRecordCountAt, 2); }, true);
  mutate(14, "a count one less", base, [&](Blob& b) { put<uint64_t>(b, l.records_at + kCheckpointRecord + kRecordCountAt, 1); }, true);
  mutate(14, "a count 2^64 - 1", base, [&](Blob& b) { put<uint64_t>(b, l.records_at + kRecordCountAt, ~0ull); }, true);
  mutate(14, "the flag set on a plain blob", plain, [](Blob& b) { put<uint32_t>(b, 64, 1); }, false);
  // what the check does not look at: these pass
  mutate(0, "a key", base, [&](Blob& b) { put<int32_t>(b, l.records_at + 4, 123456); }, true);
  mutate(0, "a mean, NaN", base, [&](Blob& b) { put<double>(b, l.records_at + 16, std::numeric_limits<double>::quiet_NaN()); }, true);
  mutate(0, "a covariance, asymmetric", base, [&](Blob& b) { put<double>(b, l.records_at + 48, -77.0); }, true);
  mutate(0, "a count without raw points", plain, [&](Blob& b) { put<uint64_t>(b, l.records_at + kRecordCountAt, 1000); }, true);
  mutate(0, "a raw point", base, [&](Blob& b) { put<double>(b, l.raw_at, 1e300); }, true);

  // ---- every truncation length of one small blob
  for (size_t n = 0; n < base.size(); ++n) {
    const int rule = offer(base, n);
    ++truncations;
    if (rule == 0 || (n >= kCheckpointHeader && rule != 8) || (n < kCheckpointHeader && rule != 1)) {
      std::printf("MISMATCH truncated to %zu: rule %d\n", n, rule);
      ++g_mismatch;
    }
  }
  // ---- every single flipped bit of it
  for (size_t bit = 0; bit < 8 * base.size(); ++bit) {
    Blob b = base;
    b[bit / 8] ^= (unsigned char)(1u << (bit % 8));
    const int rule = offer(b, b.size());
    ++flips;
    const double v = get<double>(b, 24);
    const bool in_voxel_size = bit / 8 >= 24 && bit / 8 < 32;
    const bool may_pass = in_voxel_size && std::isfinite(v) && v > 0.0;   // see the head of this file
    if (may_pass) ++harmless;
    if ((rule == 0) != may_pass) {
      std::printf("MISMATCH bit %zu flipped: rule %d\n", bit, rule);
      ++g_mismatch;
    }
    if (bit / 8 >= kCheckpointHeader && rule != 9) {
      std::printf("MISMATCH payload bit %zu flipped: rule %d, expected 9\n", bit, rule);
      ++g_mismatch;
    }
  }
  for (int r = 1; r <= VGICP_CHECKPOINT_RULES; ++r)
    if (g_fired[r] == 0) {
      std::printf("MISMATCH rule %d never fired\n", r);
      ++g_mismatch;
    }
  if (g_out) std::fclose(g_out);
  std::printf("%s built %ld mutations %ld truncations %ld flips %ld harmless %ld offered %ld passed %ld", g_mismatch ? "FAILED" : "ok", built,
              mutations, truncations, flips, harmless, g_offered, g_fired[0]);
  for (int r = 1; r <= VGICP_CHECKPOINT_RULES; ++r) std::printf(" rule %d %ld", r, g_fired[r]);
  std::printf("\n");
  return g_mismatch ? 1 : 0;
}
