// vgicp_table.hip — the voxel table's own kernels: clearing, batched upsert, rebuild into a larger table, erase, the
// voxel-key test hook, correspondence materialisation and the dense record copy.  None of them is part of a
// registration round; the probe they share with the rounds (find_voxel, voxel_hash) is vgicp_device_fn.h's.
//
// Reference behaviour each kernel reproduces (paths relative to the reference checkout):
//   upsert/erase    the effect of LocalMap::updateLocalMap's insert and evict loops on the data the
//                   path reads (src/LocalMap.cpp:47-72), mirrored from host-computed voxel values
//   match kernels   LocalMap::correspondenceMatching with materialised output (src/LocalMap.cpp:78-112)
#include "vgicp_device.h"
#include "vgicp_device_fn.h"

namespace vgicp {
namespace {

__global__ void table_clear_kernel(VoxelRecord* table, uint64_t slots) {
  // 8 threads per record, 16 B each
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= slots * 8) return;
  reinterpret_cast<int4*>(table)[g] = make_int4(0, 0, 0, 0);
}

// Batched upsert / rebuild in TWO launches, so that nothing inside a launch depends on what another workgroup of the
// same launch wrote except the one state word that is claimed by compare-and-swap:
//   claim   one thread per record: walk the probe sequence with ONE compare-and-swap per slot (EMPTY -> LOCKED).
//           Won: the slot is this record's (fresh).  Lost to LOCKED: another key of this batch (keys are unique within
//           a batch) — next slot.  Lost to FULL: a record from an earlier launch, its key is plain memory by now —
//           mine (update in place) or next slot.  The slot index (and the fresh bit) goes to a scratch word per record.
//   write   eight lanes per record, 16 bytes each (a record is one 128-byte line: {key, state} | mean + covariance =
//           six 16-byte pieces | {count, spare}): plain coalesced stores, FULL included — the kernel boundary publishes.
// One thread per record with a CAS, a release store and twelve scalar 8-byte stores into a random line measured 1.8 ms
// per million voxels (profiles/r08_c2_kernel_stats.csv); eight lanes per record in ONE launch needs the key visible
// before the state inside the launch: write-through key stores + wait cost 1.45 ms, a release fence per wave (it writes
// the XCD's L2 back) 5.5 ms.
// kClaimFresh / kClaimFailed: vgicp_device.h (the raw-point store reads the rehash's scratch words too)

// claim_slot: vgicp_device_fn.h (the map levels' claim launch, vgicp_levels.hip, walks the same way)

__global__ __launch_bounds__(256) void upsert_claim_kernel(VoxelRecord* table, uint32_t mask, uint32_t n,
                                                           const int32_t* __restrict__ keys, uint32_t* __restrict__ claimed,
                                                           uint32_t* counters) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t c = 0;
  if (i < n) {
    c = claim_slot(table, mask, keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2]);
    claimed[i] = c;
  }
  wave_count(&counters[0], i < n && c != kClaimFailed && (c & kClaimFresh) != 0);
  wave_count(&counters[1], i < n && c == kClaimFailed);
}

__global__ __launch_bounds__(256) void upsert_write_kernel(VoxelRecord* table, uint32_t n, const uint32_t* __restrict__ claimed,
                                                           const int32_t* __restrict__ keys, const double* __restrict__ means,
                                                           const double* __restrict__ covs) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = t >> 3, sub = t & 7u;
  if (i >= n) return;
  const uint32_t c = claimed[i];
  if (c == kClaimFailed) return;
  const bool fresh = (c & kClaimFresh) != 0;
  double2* line = reinterpret_cast<double2*>(table + (c & ~kClaimFresh));
  if (sub == 0) {
    if (fresh) reinterpret_cast<int4*>(line)[0] = make_int4(keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2], SLOT_FULL);
  } else if (sub == 7) {
    // numPoints of a voxel mirrored from the host is not part of the batch: a new record starts at 1
    if (fresh) reinterpret_cast<ulonglong2*>(line)[7] = make_ulonglong2(1ull, 0ull);
  } else {
    // piece `sub` of the payload: doubles 2 (sub - 1), 2 (sub - 1) + 1 of {mean[3], cov[9]}
    const uint32_t p = 2u * (sub - 1u);
    double2 piece;
    piece.x = p < 3u ? means[3 * (size_t)i + p] : covs[9 * (size_t)i + (p - 3u)];
    piece.y = p + 1u < 3u ? means[3 * (size_t)i + p + 1u] : covs[9 * (size_t)i + (p + 1u - 3u)];
    line[sub] = piece;
  }
}

// The rebuild into a larger table: one thread per OLD slot claims (the new table holds nothing else, every claim wins a
// fresh slot), eight lanes per old slot then copy the 128-byte line.
__global__ __launch_bounds__(256) void rehash_claim_kernel(const VoxelRecord* __restrict__ old_table, uint64_t old_slots,
                                                           VoxelRecord* table, uint32_t mask, uint32_t* __restrict__ claimed,
                                                           uint32_t* counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t c = 0;
  bool full = false;
  if (i < old_slots) {
    const int4 head = *reinterpret_cast<const int4*>(old_table + i);
    full = head.w == SLOT_FULL;
    c = full ? claim_slot(table, mask, head.x, head.y, head.z) : kClaimFailed;
    claimed[i] = c;
  }
  wave_count(&counters[0], full && c != kClaimFailed);
  wave_count(&counters[1], full && c == kClaimFailed);
}

__global__ __launch_bounds__(256) void rehash_write_kernel(const VoxelRecord* __restrict__ old_table, uint64_t old_slots,
                                                           VoxelRecord* table, const uint32_t* __restrict__ claimed) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i = t >> 3;
  const uint32_t sub = (uint32_t)(t & 7u);
  if (i >= old_slots) return;
  const uint32_t c = claimed[i];
  if (c == kClaimFailed) return;
  double2 piece = reinterpret_cast<const double2*>(old_table + i)[sub];
  if (sub == 7) piece.y = 0.0;   // the spare word (per-voxel list head of an insertion) does not travel
  reinterpret_cast<double2*>(table + (c & ~kClaimFresh))[sub] = piece;
}

__global__ void erase_kernel(VoxelRecord* table, uint32_t mask, uint32_t n,
                             const int32_t* __restrict__ keys, uint32_t* counters) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t kx = keys[3 * (size_t)i], ky = keys[3 * (size_t)i + 1], kz = keys[3 * (size_t)i + 2];
  uint32_t slot = voxel_hash(kx, ky, kz) & mask;
  bool erased = false;
  for (uint32_t probes = 0; probes <= mask; ++probes) {
    VoxelRecord* rec = table + slot;
    const int32_t state = rec->state;
    if (state == SLOT_EMPTY) break;
    if (state == SLOT_FULL && rec->key[0] == kx && rec->key[1] == ky && rec->key[2] == kz) {
      // duplicates in the batch race here: exactly one CAS wins and counts
      int32_t expected = SLOT_FULL;
      erased = __hip_atomic_compare_exchange_strong(&rec->state, &expected, SLOT_TOMB, __ATOMIC_RELAXED,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    slot = (slot + 1) & mask;
  }
  wave_count(&counters[0], erased);
}

__global__ void voxel_index_kernel(const double* __restrict__ pts, uint32_t n, double voxel_size,
                                   int32_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // the division-free form the loop kernels use (exact, see voxel_coord_fast): this hook is how tests pin it
  // ... and the persistent launch's shortcut "still in last round's voxel?" (same_voxel_coord): it may say no for
  // the true key (the caller then makes the key), but a yes for any OTHER key would be a wrong correspondence — the
  // hook poisons the key it returns in that case, so the same tests pin both functions.
  const double inv_voxel = 1.0 / voxel_size;
  const double same_margin = 0x1p-20 * voxel_size;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double x = pts[3 * (size_t)i + k];
    int32_t key = voxel_coord_fast(x, voxel_size, inv_voxel);
    bool wrong_yes = false;
#pragma unroll
    for (int d = 1; d <= 2; ++d) {
      if (key <= INT32_MAX - d) wrong_yes = wrong_yes || same_voxel_coord(x, key + d, voxel_size, same_margin);
      if (key >= INT32_MIN + d) wrong_yes = wrong_yes || same_voxel_coord(x, key - d, voxel_size, same_margin);
    }
    keys[3 * (size_t)i + k] = wrong_yes ? INT32_MIN : key;
  }
}

// ---- correspondence materialisation: count per block, scan block counts, compact ----
constexpr int kMatchBlock = 256;

__device__ __forceinline__ const VoxelRecord* match_point(const double* pts, uint32_t i, uint32_t n,
                                                          const VoxelRecord* table, uint32_t mask,
                                                          double voxel_size) {
  if (i >= n) return nullptr;
  const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  return find_voxel(table, mask, voxel_coord(x, voxel_size), voxel_coord(y, voxel_size),
                    voxel_coord(z, voxel_size));
}

__global__ __launch_bounds__(kMatchBlock) void match_count_kernel(
    const double* __restrict__ pts, uint32_t n, const VoxelRecord* __restrict__ table, uint32_t mask,
    double voxel_size, uint32_t* __restrict__ block_counts) {
  const uint32_t i = blockIdx.x * kMatchBlock + threadIdx.x;
  const bool hit = match_point(pts, i, n, table, mask, voxel_size) != nullptr;
  const int total = __syncthreads_count(hit ? 1 : 0);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = (uint32_t)total;
}

// Exclusive scan of block_counts in place by one workgroup; total -> *total_out.
__global__ __launch_bounds__(1024) void match_scan_kernel(uint32_t* counts, uint32_t nb,
                                                          uint32_t* total_out) {
  __shared__ uint32_t wave_sum[16];
  __shared__ uint32_t carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nb; base += 1024) {
    const uint32_t idx = base + tid;
    const uint32_t val = idx < nb ? counts[idx] : 0u;
    uint32_t incl = val;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t w = 0; w < wave; ++w) before += wave_sum[w];
    if (idx < nb) counts[idx] = before + incl - val;
    __syncthreads();
    if (tid == 1023) carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) *total_out = carry;
}

__global__ __launch_bounds__(kMatchBlock) void match_write_kernel(
    const double* __restrict__ pts, const double* __restrict__ covs, uint32_t n,
    const VoxelRecord* __restrict__ table, uint32_t mask, double voxel_size,
    const uint32_t* __restrict__ block_offsets, double* __restrict__ src_points,
    double* __restrict__ src_covs, double* __restrict__ map_points, double* __restrict__ map_covs,
    uint64_t* __restrict__ src_index) {
  __shared__ uint32_t wave_hits[kMatchBlock / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t i = blockIdx.x * kMatchBlock + tid;
  const VoxelRecord* rec = match_point(pts, i, n, table, mask, voxel_size);
  const unsigned long long ballot = __ballot(rec != nullptr);
  if (lane == 0) wave_hits[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (rec == nullptr) return;
  uint32_t pos = block_offsets[blockIdx.x] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
  for (uint32_t w = 0; w < wave; ++w) pos += wave_hits[w];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    src_points[3 * (size_t)pos + k] = pts[3 * (size_t)i + k];
    map_points[3 * (size_t)pos + k] = rec->mean[k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    src_covs[9 * (size_t)pos + k] = covs[9 * (size_t)i + k];
    map_covs[9 * (size_t)pos + k] = rec->cov[k];
  }
  if (src_index) src_index[pos] = i;
}

// ---- dense copy of the FULL records (count per block -> scan -> copy) ----
constexpr int kDenseBlock = 256;
__global__ __launch_bounds__(kDenseBlock) void dense_count_kernel(const VoxelRecord* __restrict__ table, uint64_t slots,
                                                                  uint32_t* __restrict__ block_counts) {
  const uint64_t i = (uint64_t)blockIdx.x * kDenseBlock + threadIdx.x;
  const bool full = i < slots && table[i].state == SLOT_FULL;
  const int total = __syncthreads_count(full ? 1 : 0);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = (uint32_t)total;
}
__global__ __launch_bounds__(kDenseBlock) void dense_write_kernel(VoxelRecord* table, uint64_t slots,
                                                                  const uint32_t* __restrict__ block_offsets,
                                                                  VoxelRecord* __restrict__ dense, uint64_t capacity) {
  __shared__ uint32_t wave_hits[kDenseBlock / 64];
  __shared__ uint32_t src[kDenseBlock];   // local slot numbers of the block's FULL records, in slot order
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * kDenseBlock + tid;
  const bool full = i < slots && table[i].state == SLOT_FULL;
  const unsigned long long ballot = __ballot(full);
  if (lane == 0) wave_hits[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  uint32_t rank = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull)), total = 0;
  for (uint32_t w = 0; w < kDenseBlock / 64; ++w) {
    if (w < wave) rank += wave_hits[w];
    total += wave_hits[w];
  }
  const uint32_t base = block_offsets[blockIdx.x];
  if (full) {
    src[rank] = tid;
    reinterpret_cast<uint32_t*>(&table[i].reserved)[1] = base + rank;   // where this record's copy lives
  }
  __syncthreads();
  // eight lanes per record, 16 bytes each: coalesced 128-byte lines both ways
  // never beyond the allocation (the host sizes it for every record a pending insertion may still add; this is the belt)
  for (uint32_t r = tid >> 3; r < total && (uint64_t)base + r < capacity; r += kDenseBlock / 8) {
    const double2 piece = reinterpret_cast<const double2*>(table + ((uint64_t)blockIdx.x * kDenseBlock + src[r]))[tid & 7u];
    reinterpret_cast<double2*>(dense + base + r)[tid & 7u] = piece;
  }
}

}  // namespace

hipError_t launch_table_clear(hipStream_t s, VoxelRecord* table, uint64_t slots) {
  counted_launch(table_clear_kernel, dim3(blocks_for(slots * 8, 256)), dim3(256), 0, s, table, slots);
  return hipGetLastError();
}

uint32_t table_dense_blocks(uint64_t slots) { return blocks_for(slots, kDenseBlock); }

hipError_t launch_table_dense(hipStream_t s, VoxelRecord* table, uint64_t slots, VoxelRecord* dense, uint64_t dense_capacity,
                              uint32_t* block_counts) {
  const uint32_t nb = table_dense_blocks(slots);
  counted_launch(dense_count_kernel, dim3(nb), dim3(kDenseBlock), 0, s, table, slots, block_counts);
  counted_launch(match_scan_kernel, dim3(1), dim3(1024), 0, s, block_counts, nb, block_counts + nb);
  counted_launch(dense_write_kernel, dim3(nb), dim3(kDenseBlock), 0, s, table, slots, block_counts, dense, dense_capacity);
  return hipGetLastError();
}

hipError_t launch_upsert(hipStream_t s, VoxelRecord* table, uint32_t mask, uint32_t n,
                         const int32_t* keys, const double* means, const double* covs,
                         uint32_t* counters, uint32_t* claimed) {
  if (n == 0) return hipSuccess;
  counted_launch(upsert_claim_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, table, mask, n, keys, claimed, counters);
  counted_launch(upsert_write_kernel, dim3(blocks_for((uint64_t)n * 8, 256)), dim3(256), 0, s, table, n, claimed, keys, means,
                 covs);
  return hipGetLastError();
}

hipError_t launch_erase(hipStream_t s, VoxelRecord* table, uint32_t mask, uint32_t n,
                        const int32_t* keys, uint32_t* counters) {
  if (n == 0) return hipSuccess;
  counted_launch(erase_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, table, mask, n, keys, counters);
  return hipGetLastError();
}

hipError_t launch_rehash(hipStream_t s, const VoxelRecord* old_table, uint64_t old_slots,
                         VoxelRecord* table, uint32_t mask, uint32_t* counters, uint32_t* claimed) {
  counted_launch(rehash_claim_kernel, dim3(blocks_for(old_slots, 256)), dim3(256), 0, s, old_table, old_slots, table, mask,
                 claimed, counters);
  counted_launch(rehash_write_kernel, dim3(blocks_for(old_slots * 8, 256)), dim3(256), 0, s, old_table, old_slots, table,
                 claimed);
  return hipGetLastError();
}

hipError_t launch_voxel_index(hipStream_t s, const double* points_aos, uint32_t n, double voxel_size,
                              int32_t* keys) {
  if (n == 0) return hipSuccess;
  counted_launch(voxel_index_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, points_aos, n, voxel_size, keys);
  return hipGetLastError();
}

uint32_t match_blocks(uint32_t n) { return blocks_for(n, kMatchBlock); }

hipError_t launch_match(hipStream_t s, const double* points_aos, const double* covs_aos, uint32_t n,
                        const VoxelRecord* table, uint32_t mask, double voxel_size,
                        uint32_t* block_counts, uint32_t* total, double* src_points,
                        double* src_covs, double* map_points, double* map_covs, uint64_t* src_index) {
  const uint32_t nb = match_blocks(n);
  counted_launch(match_count_kernel, dim3(nb), dim3(kMatchBlock), 0, s, points_aos, n, table, mask, voxel_size, block_counts);
  counted_launch(match_scan_kernel, dim3(1), dim3(1024), 0, s, block_counts, nb, total);
  counted_launch(match_write_kernel, dim3(nb), dim3(kMatchBlock), 0, s, points_aos, covs_aos, n, table, mask, voxel_size,
                 block_counts, src_points, src_covs, map_points, map_covs, src_index);
  return hipGetLastError();
}

}  // namespace vgicp
