// GPU check of the library's sort (eskf_lio_amd/csrc/vgicp_sort.h) against std::stable_sort, for both key types it is
// used with: 64-bit Morton codes (the scan preparation) and 32-bit voxel slots (the map insertion).  Sizes around every
// boundary of the plan (one tile, a tile's end, a group's end, a level more, up to the 8 M-point limit of a scan), keys
// with long runs of equal values (a scan's voxel codes), all equal, already sorted, reversed, random keys of the full
// width, few distinct keys in the high and low bits, and keys that mix ordinary values with the largest key the sort
// accepts (~K(0) - 1: the insertion's table-full slot) at the end, where the padding of a partial tile is.  Built by the
// module's Makefile (`make sort_check`) into eskf_lio_amd/lib/, run by tests/test_gpu_parity.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../eskf_lio_amd/csrc/vgicp_sort.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

static unsigned long long rng_state = 0x2545F4914F6CDD1Dull;
static unsigned long long rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

constexpr int kKinds = 7;

// key i of n of the given kind; every key lies below ~K(0), the sort's padding
template <typename K>
static K make_key(int kind, uint32_t i, uint32_t n) {
  constexpr bool wide = sizeof(K) == 8;
  const K top = ~K(0) - 1;
  switch (kind) {
    case 0: return (K)(rng() % (n / 6 + 1));                                        // ~6 pairs per key: voxel codes
    case 1: return wide ? (K)(rng() >> 1) : (K)(rng() % ~K(0));                      // 63 random bits / 32 random bits
    case 2: return 42;                                                              // all equal: the order is the index order
    case 3: return i / 3;                                                           // sorted already
    case 4: return (n - i) / 5;                                                     // reversed
    case 5: return (K)(rng() % 7) << (wide ? 60 : 29) | (K)(rng() % 3);             // few distinct keys, high and low bits
    default: return i >= n - n / 4 - 1 || rng() % 8 == 0 ? top : (K)(rng() % (n / 6 + 1));   // the largest key, last
  }
}

// sort_check time <n> [kind] [key bits]: the launches of one sort, timed (for rocprofv3 --kernel-trace --stats)
template <typename K>
static int time_sort(uint32_t n, int kind) {
  std::vector<K> keys(n);
  // kind 0: random keys, ~6 pairs each; kind 1: a walk (consecutive pairs have nearby keys, as a sweep's points do)
  unsigned long long walk = 1ull << 40;
  for (uint32_t i = 0; i < n; ++i) {
    if (kind == 0) keys[i] = make_key<K>(0, i, n);
    else { walk += (rng() % 2001) - 1000; if (i % 900 == 0) walk = (1ull << 40) + rng() % 3000000; keys[i] = (K)((walk >> 3) % (~K(0))); }
  }
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  const size_t kbytes = sizeof(K);
  K *ka, *kb, *k0; uint32_t *ia, *ib, *i0; void* split;
  CK(hipMalloc(&ka, n * kbytes)); CK(hipMalloc(&kb, n * kbytes)); CK(hipMalloc(&k0, n * kbytes));
  CK(hipMalloc(&ia, n * 4ull)); CK(hipMalloc(&ib, n * 4ull)); CK(hipMalloc(&i0, n * 4ull));
  CK(hipMalloc(&split, vgicp::sortk::split_bytes(n, kbytes)));
  CK(hipMemcpy(k0, keys.data(), n * kbytes, hipMemcpyHostToDevice));
  CK(hipMemcpy(i0, idx.data(), n * 4ull, hipMemcpyHostToDevice));
  hipStream_t s; CK(hipStreamCreate(&s));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float total = 0;
  for (int rep = 0; rep < 220; ++rep) {
    CK(hipMemcpyAsync(ka, k0, n * kbytes, hipMemcpyDeviceToDevice, s));
    CK(hipMemcpyAsync(ia, i0, n * 4ull, hipMemcpyDeviceToDevice, s));
    CK(hipEventRecord(e0, s));
    CK(vgicp::sortk::sort_pairs(ka, ia, kb, ib, split, n, s));
    CK(hipEventRecord(e1, s));
    CK(hipStreamSynchronize(s));
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    if (rep >= 20) total += ms;
  }
  std::printf("n = %u, kind %d, %d-bit keys: %.2f us per sort (%u launches)\n", n, kind, (int)(8 * kbytes), total / 200 * 1e3,
              vgicp::sortk::launches_for(n));
  return 0;
}

// every size and kind against std::stable_sort; ka / kb hold cap keys of 8 bytes, ia / ib cap indices
template <typename K>
static int check(void* ka_, void* kb_, uint32_t* ia, uint32_t* ib, void* split, uint32_t cap, hipStream_t s, int& checked) {
  const uint32_t sizes[] = {1, 2, 3, 255, 257, 1023, 1024, 1025, 2048, 2049, 4097, 8191, 8192, 8193, 10131, 16385, 60000, 65535,
                            65536, 65537, 100000, 131073, 262144, 262145, 300001, 1000003, 1048577,
                            4194304, 4194305, 6000001, 8388608};   // 8 merge levels: the sizes of a scan on the 8-item branch
  K* ka = static_cast<K*>(ka_);
  K* kb = static_cast<K*>(kb_);
  K untouched;
  std::memset(&untouched, 0xEE, sizeof(K));
  for (uint32_t n : sizes) {
    for (int kind = 0; kind < kKinds; ++kind) {
      if (n > 300001 && kind > 1) continue;
      std::vector<K> keys(n);
      for (uint32_t i = 0; i < n; ++i) keys[i] = make_key<K>(kind, i, n);
      std::vector<uint32_t> idx(n);
      std::iota(idx.begin(), idx.end(), 0u);
      CK(hipMemcpyAsync(ka, keys.data(), n * sizeof(K), hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(ia, idx.data(), n * 4ull, hipMemcpyHostToDevice, s));
      CK(hipMemsetAsync(kb, 0xEE, cap * sizeof(K), s));
      CK(hipMemsetAsync(ib, 0xEE, cap * 4ull, s));
      CK(vgicp::sortk::sort_pairs(ka, ia, kb, ib, split, n, s));
      std::vector<K> got_k(n + 1);
      std::vector<uint32_t> got_i(n + 1);
      CK(hipMemcpyAsync(got_k.data(), kb, (n + 1) * sizeof(K), hipMemcpyDeviceToHost, s));
      CK(hipMemcpyAsync(got_i.data(), ib, (n + 1) * 4ull, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
      for (uint32_t i = 0; i < n; ++i) {
        if (got_i[i] != idx[i] || got_k[i] != keys[idx[i]]) {
          std::printf("%d-bit keys, n = %u, kind %d: position %u holds (%llu, %u), expected (%llu, %u)\n", (int)(8 * sizeof(K)), n,
                      kind, i, (unsigned long long)got_k[i], got_i[i], (unsigned long long)keys[idx[i]], idx[i]);
          return 1;
        }
      }
      if (got_k[n] != untouched || got_i[n] != 0xEEEEEEEEu) {
        std::printf("%d-bit keys, n = %u, kind %d: wrote past the end\n", (int)(8 * sizeof(K)), n, kind);
        return 1;
      }
      ++checked;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 2) {
    const uint32_t n = (uint32_t)std::atoi(argv[2]);
    const int kind = argc > 3 ? std::atoi(argv[3]) : 0;
    const int bits = argc > 4 ? std::atoi(argv[4]) : 64;
    if (bits != 32 && bits != 64) { std::printf("key bits: 32 or 64\n"); return 2; }
    return bits == 32 ? time_sort<uint32_t>(n, kind) : time_sort<unsigned long long>(n, kind);
  }
  const uint32_t cap = 8388608 + 8;
  void *ka, *kb;
  uint32_t *ia, *ib;
  CK(hipMalloc(&ka, cap * 8ull)); CK(hipMalloc(&kb, cap * 8ull)); CK(hipMalloc(&ia, cap * 4ull)); CK(hipMalloc(&ib, cap * 4ull));
  void* split;
  CK(hipMalloc(&split, vgicp::sortk::split_bytes(cap, 8)));
  hipStream_t s;
  CK(hipStreamCreate(&s));
  int checked = 0;
  int rc = check<unsigned long long>(ka, kb, ia, ib, split, cap, s, checked);
  if (rc == 0) rc = check<uint32_t>(ka, kb, ia, ib, split, cap, s, checked);
  if (rc != 0) return rc;
  std::printf("ok: %d sorts (64- and 32-bit keys), %u launches for 60 000 pairs, %u for 1 000 000\n", checked,
              vgicp::sortk::launches_for(60000), vgicp::sortk::launches_for(1000000));
  return 0;
}
