// CPU check of the voxel table's hash (eskf_lio_amd/csrc/vgicp_device_fn.h: fmix32, voxel_hash) — compiled by hipcc,
// no device call.  Prints "x y z hash" for a fixed list of keys: zero, small keys of both signs, the int32 edges
// (+-2^31 and their neighbours) in every position, and keys from a fixed 64-bit LCG.  tests/test_voxel_table.py
// compares every line with its numpy restatement of the hash, from which the GPU tests craft colliding keys.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../eskf_lio_amd/csrc/vgicp_device_fn.h"

int main() {
  std::vector<int32_t> edges = {0, 1, -1, 2, -2, 7, -7, 1000, -1000, 65535, -65536, 0x40000000, -0x40000000,
                                INT32_MAX, INT32_MAX - 1, INT32_MIN, INT32_MIN + 1};
  std::vector<int32_t> keys;
  for (int32_t x : edges)
    for (int32_t y : edges)
      for (int32_t z : {edges[0], edges[2], edges[13], edges[15], y, x}) keys.insert(keys.end(), {x, y, z});
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 3 * 2000; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    keys.push_back((int32_t)(uint32_t)(s >> 32));
  }
  for (size_t i = 0; i < keys.size(); i += 3)
    std::printf("%d %d %d %u\n", keys[i], keys[i + 1], keys[i + 2], vgicp::voxel_hash(keys[i], keys[i + 1], keys[i + 2]));
  return 0;
}
