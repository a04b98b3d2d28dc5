// vgicp_levels.hip — the map's coarser levels (include/vgicp_hip_map_levels.h): level l, voxel size voxel_size * 2^l,
// built from level l-1 alone in two launches, CLAIM and FILL.  The header has the rule operation by operation;
// tests/map_levels_reference.py restates it.  Built without FMA contraction (Makefile), and every product, sum and
// quotient of the merge is an explicit round-to-nearest intrinsic besides: the result is the restatement's bit for bit.
//
// The table's claim (claim_slot, vgicp_device_fn.h) asks that the keys claiming within one launch are unique, and up to
// eight children share a parent.  So ONE child claims for its parent: the first in octant order, which a child finds
// out by probing its lower-octant siblings (none for octant 0, on average well under one probe that hits).
// The claim leaves the slot LOCKED and writes the parent's key beside the state.  Within the claim launch nobody reads
// that key (claim_slot compares keys of FULL slots only, and a cleared table has none); the launch boundary publishes it
// to the fill launch, which finds its work by the LOCKED state: no scratch array between the two launches, and the fill
// launch is as large as the LEVEL's table, not as the finer one (a map table is sized for what it may grow to: 2 M slots
// for 29 000 voxels in the frame chain).
//
// Locate (include/vgicp_hip_map_locate.h) reads a level and lives here for the same build: its transform and its key are
// stated without FMA.  Its two kernels are below the build's.
#include <cstddef>

#include "vgicp_device.h"
#include "vgicp_device_fn.h"
#include "vgicp_locate_plan.h"

namespace vgicp {
namespace {

__device__ __forceinline__ const VoxelRecord* find_child(const VoxelRecord* fine, uint32_t fine_mask, int32_t px, int32_t py,
                                                         int32_t pz, uint32_t octant) {
  return find_voxel(fine, fine_mask, 2 * px + (int32_t)(octant & 1u), 2 * py + (int32_t)((octant >> 1) & 1u),
                    2 * pz + (int32_t)(octant >> 2));
}

// One thread per kPer slots of the finer table, a workgroup's slots interleaved so that a wave's loads stay coalesced: a
// thread issues its loads of the slot heads together and only then looks at them.  A map table is sized for what it may
// grow to and is mostly EMPTY (2 M slots for 29 000 voxels in the frame chain), so over such a table this launch is one
// 16-byte read out of every 128-byte line, and what it costs is how many of those are in flight: measured over the 2 M
// slots, 149 us with one slot per thread, 112 us with four.  Over a level's table (half full at most, 65 536 slots there)
// a thread's time is its chain of sibling probes, and four slots per thread put four chains in a row: 34 us against 18.
// So kPer = 4 from kClaimWideSlots slots on, else 1.  counters[0] += parents claimed, counters[1] += probe sequences exhausted.
constexpr uint64_t kClaimWideSlots = 1ull << 20;
template <uint32_t kPer>
__global__ __launch_bounds__(256) void level_claim_kernel(const VoxelRecord* __restrict__ fine, uint64_t fine_slots,
                                                          uint32_t fine_mask, VoxelRecord* coarse, uint32_t coarse_mask,
                                                          uint32_t* counters) {
  const uint64_t first_slot = (uint64_t)blockIdx.x * (256u * kPer) + threadIdx.x;
  int4 heads[kPer];
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint64_t i = first_slot + 256u * k;
    heads[k] = i < fine_slots ? *reinterpret_cast<const int4*>(fine + i) : make_int4(0, 0, 0, SLOT_EMPTY);
  }
  uint32_t claimed = 0, failed = 0;
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const int4 head = heads[k];
    if (head.w != SLOT_FULL) continue;
    const int32_t px = head.x >> 1, py = head.y >> 1, pz = head.z >> 1;   // arithmetic: -1 -> -1
    const uint32_t octant = (uint32_t)(head.x & 1) + 2u * (uint32_t)(head.y & 1) + 4u * (uint32_t)(head.z & 1);
    bool first = true;
    for (uint32_t o = 0; o < octant && first; ++o) first = find_child(fine, fine_mask, px, py, pz, o) == nullptr;
    if (!first) continue;
    const uint32_t c = claim_slot(coarse, coarse_mask, px, py, pz);
    if (c == kClaimFailed) {
      ++failed;
      continue;
    }
    ++claimed;
    VoxelRecord* rec = coarse + (c & ~kClaimFresh);   // LOCKED, and this thread's alone
    rec->key[0] = px;
    rec->key[1] = py;
    rec->key[2] = pz;
  }
  // one atomic per wave and counter (only where there is something to add)
  for (int d = 32; d > 0; d >>= 1) {
    claimed += (uint32_t)__shfl_down((int)claimed, d, 64);
    failed += (uint32_t)__shfl_down((int)failed, d, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (claimed) atomicAdd(&counters[0], claimed);
    if (failed) atomicAdd(&counters[1], failed);
  }
}

// Eight lanes per slot of the LEVEL's table; the groups of the LOCKED slots go on.  Lane o probes child o and loads its
// record, so the eight probe chains of a parent are in flight together; then every lane of the group reads the
// children's values across the lanes in octant order and forms the same sums; lane 0 writes the record, FULL.
__global__ __launch_bounds__(256) void level_fill_kernel(const VoxelRecord* __restrict__ fine, uint32_t fine_mask,
                                                         VoxelRecord* coarse, uint64_t coarse_slots) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t slot = t >> 3;
  const uint32_t lane = threadIdx.x & 63u, o = lane & 7u, base = lane & ~7u;
  // a group leaves as one (the slot and its state are the group's), so the lanes a group reads from below are all there
  if (slot >= coarse_slots) return;
  const int4 head = *reinterpret_cast<const int4*>(coarse + slot);
  if (head.w != SLOT_LOCKED) return;
  const int32_t px = head.x, py = head.y, pz = head.z;
  const VoxelRecord* rec = find_child(fine, fine_mask, px, py, pz, o);
  double v[12];
  unsigned long long count = 0ull;
#pragma unroll
  for (int e = 0; e < 12; ++e) v[e] = 0.0;
  if (rec) {
#pragma unroll
    for (int e = 0; e < 3; ++e) v[e] = rec->mean[e];
#pragma unroll
    for (int e = 0; e < 9; ++e) v[3 + e] = rec->cov[e];
    count = rec->count;
  }
  const uint32_t present = (uint32_t)(__ballot(rec != nullptr) >> base) & 0xFFu;
  double acc[12], only[12];
  unsigned long long total = 0ull;
  bool started = false;
#pragma unroll
  for (int e = 0; e < 12; ++e) acc[e] = only[e] = 0.0;
#pragma unroll 1   // unrolled, the 96 cross-lane reads are all scheduled up front and cost 170 registers (occupancy 2)
  for (uint32_t src = 0; src < 8u; ++src) {
    const unsigned long long n_c = __shfl(count, (int)(base + src), 64);
    const bool has = (present >> src) & 1u;
    if (has) total += n_c;
    const double w = (double)n_c;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      const double x = __shfl(v[e], (int)(base + src), 64);
      const double p = __dmul_rn(w, x);
      if (has) {
        acc[e] = started ? __dadd_rn(acc[e], p) : p;   // the sum starts from the first child's product
        if (!started) only[e] = x;
      }
    }
    started = started || has;
  }
  if (o != 0u) return;
  const bool single = __popc(present) == 1;
  const double n = (double)total;
  double out[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) out[e] = single ? only[e] : __ddiv_rn(acc[e], n);   // one child: its bits
  VoxelRecord* dst = coarse + slot;
  double2* line = reinterpret_cast<double2*>(dst);
#pragma unroll
  for (int piece = 1; piece < 7; ++piece) line[piece] = make_double2(out[2 * (piece - 1)], out[2 * (piece - 1) + 1]);
  reinterpret_cast<ulonglong2*>(dst)[7] = make_ulonglong2(total, 0ull);
  dst->state = SLOT_FULL;   // the kernel boundary publishes
}

// ---- locate (include/vgicp_hip_map_locate.h states the rule operation by operation; this restates it) ----
// A workgroup has kLocateChunk points that take part, at one pose.  Their keys are made ONCE, by one lane each, and kept
// in LDS; then the (point, cell) pairs of the chunk are dealt to the threads in turn, cell fastest, so that the lanes
// of a wave hold 64 independent probes whatever the window's size (a window of one cell keeps 64 points in flight, one of
// 3 969 cells 64 cells of one point), and neighbouring lanes probe neighbouring keys.  A thread's pair advances by
// kLocateBlock pairs per turn: the step is split into the mixed radix (x, y, z, point) once, and a turn is three
// additions with a carry each, no division.  A probe reads the 16-byte head of a record (find_voxel); a hit is one LDS
// integer atomic on the window's histogram; the non-zero cells go to the plane as integer atomics without a return.
// A first version: one probe per lane and turn, the waves of a CU's workgroups hide the probe's latency between them.
static_assert(sizeof(vgicp_locate_best) == 160 && offsetof(vgicp_locate_best, pose) == 32, "vgicp_locate_best: 160 bytes");
__global__ __launch_bounds__(kLocateBlock) void locate_score_kernel(LocateArgs a) {
  __shared__ uint32_t hist[VGICP_LOCATE_MAX_CELLS];
  __shared__ int4 keys[kLocateChunk];   // w: 1 where the key is defined
  const uint32_t tid = threadIdx.x, pose = blockIdx.y;
  for (uint32_t c = tid; c < a.cells; c += kLocateBlock) hist[c] = 0u;
  const uint32_t first = blockIdx.x * kLocateChunk;
  const uint32_t count = min(kLocateChunk, a.participants - first);
  if (tid < kLocateChunk) {   // whole waves
    bool skip = false;
    if (tid < count) {
      const double* m = a.poses + 16 * (size_t)pose;   // column-major 4 x 4
      const double R[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
      const double t[3] = {m[12], m[13], m[14]};
      const double* p = a.points_aos + 3 * ((size_t)(first + tid) * a.stride);
      double e[3];
      int32_t k[3];
      transform_point(R, t, p[0], p[1], p[2], e);
      skip = !carve_key(e, a.voxel_size, k);
      keys[tid] = make_int4(k[0], k[1], k[2], skip ? 0 : 1);
    }
    wave_count(a.skipped + pose, skip);
  }
  __syncthreads();
  const uint32_t W = 2u * (uint32_t)a.window[0] + 1u, H = 2u * (uint32_t)a.window[1] + 1u, D = 2u * (uint32_t)a.window[2] + 1u;
  uint32_t x = tid % W, r = tid / W;
  uint32_t y = r % H;
  r /= H;
  uint32_t z = r % D, p = r / D;
  const uint32_t sx = kLocateBlock % W, r1 = kLocateBlock / W, sy = r1 % H, r2 = r1 / H, sz = r2 % D, sp = r2 / D;
  while (p < count) {
    const int4 key = keys[p];
    if (key.w != 0 &&
        find_voxel(a.table, a.mask, key.x + ((int32_t)x - a.window[0]), key.y + ((int32_t)y - a.window[1]), key.z + ((int32_t)z - a.window[2])))
      atomicAdd(&hist[(z * H + y) * W + x], 1u);
    x += sx;
    if (x >= W) { x -= W; ++y; }
    y += sy;
    if (y >= H) { y -= H; ++z; }
    z += sz;
    if (z >= D) { z -= D; ++p; }
    p += sp;
  }
  __syncthreads();
  uint32_t* plane = a.plane + (size_t)pose * a.cells;
  for (uint32_t c = tid; c < a.cells; c += kLocateBlock) {
    const uint32_t v = hist[c];
    if (v) (void)__hip_atomic_fetch_add(plane + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One workgroup per pose.  (hits << 32 | ~cell) orders the cells by hits and then by the LOWER index, so the maximum of
// that word over the plane is the answer; a thread without a cell holds 0, which loses to every cell.
__global__ __launch_bounds__(kLocateBlock) void locate_best_kernel(LocateArgs a, vgicp_locate_best* out) {
  __shared__ unsigned long long parts[kLocateBlock / 64];
  const uint32_t tid = threadIdx.x, pose = blockIdx.x;
  const uint32_t* plane = a.plane + (size_t)pose * a.cells;
  unsigned long long best = 0ull;
  for (uint32_t c = tid; c < a.cells; c += kLocateBlock) {
    const unsigned long long cand = ((unsigned long long)plane[c] << 32) | (unsigned long long)(0xFFFFFFFFu - c);
    best = cand > best ? cand : best;
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_down(best, d, 64);
    best = other > best ? other : best;
  }
  if ((tid & 63u) == 0u) parts[tid >> 6] = best;
  __syncthreads();
  if (tid != 0u) return;
  for (uint32_t w = 1; w < kLocateBlock / 64; ++w) best = parts[w] > best ? parts[w] : best;
  const uint32_t cell = 0xFFFFFFFFu - (uint32_t)best;
  const uint32_t W = 2u * (uint32_t)a.window[0] + 1u, H = 2u * (uint32_t)a.window[1] + 1u;
  const int32_t d[3] = {(int32_t)(cell % W) - a.window[0], (int32_t)((cell / W) % H) - a.window[1],
                        (int32_t)(cell / (W * H)) - a.window[2]};
  const uint32_t skipped = a.skipped[pose];
  vgicp_locate_best* o = out + pose;
  o->hits = (uint32_t)(best >> 32);
  o->cell = cell;
  o->points = a.participants - skipped;
  o->skipped = skipped;
  o->reserved = 0u;
  const double* m = a.poses + 16 * (size_t)pose;
  for (int e = 0; e < 16; ++e) o->pose[e] = m[e];
  for (int e = 0; e < 3; ++e) {
    o->offset[e] = d[e];
    o->pose[12 + e] = __dadd_rn(m[12 + e], __dmul_rn((double)d[e], a.voxel_size));   // one product, one sum
  }
}

}  // namespace

hipError_t launch_locate(hipStream_t s, const LocateArgs& a, uint32_t poses, void* best) {
  if (a.participants != 0u)
    counted_launch(locate_score_kernel, dim3(locate_chunks(a.participants), poses), dim3(kLocateBlock), 0, s, a);
  counted_launch(locate_best_kernel, dim3(poses), dim3(kLocateBlock), 0, s, a, static_cast<vgicp_locate_best*>(best));
  return hipGetLastError();
}

hipError_t launch_level_build(hipStream_t s, const VoxelRecord* fine, uint64_t fine_slots, VoxelRecord* coarse,
                              uint64_t coarse_slots, uint32_t* counters) {
  const uint32_t fine_mask = (uint32_t)(fine_slots - 1), coarse_mask = (uint32_t)(coarse_slots - 1);
  if (fine_slots >= kClaimWideSlots)
    counted_launch(level_claim_kernel<4>, dim3(blocks_for(fine_slots, 256 * 4)), dim3(256), 0, s, fine, fine_slots, fine_mask, coarse,
                   coarse_mask, counters);
  else
    counted_launch(level_claim_kernel<1>, dim3(blocks_for(fine_slots, 256)), dim3(256), 0, s, fine, fine_slots, fine_mask, coarse,
                   coarse_mask, counters);
  counted_launch(level_fill_kernel, dim3(blocks_for(coarse_slots * 8, 256)), dim3(256), 0, s, fine, fine_mask, coarse,
                 coarse_slots);
  return hipGetLastError();
}

}  // namespace vgicp
