// vgicp_mapupdate.hip — LocalMap::updateLocalMap's insert and evict loops on the device
// (reference src/LocalMap.cpp:44-72, include/ESKF_LIO/LocalMap.hpp:63-89).
//
// The reference inserts serially: for every point in scan order, find its voxel; a missing voxel is
// constructed from the point (mean = p, covariance = C, numPoints = 1), an existing one takes
// Voxel::addPoint — mean <- (n*mean + p)/(n+1), covariance likewise, while numPoints < maxNumPoints.
// The result depends on the ORDER of the points inside a voxel, so the device version keeps it:
//   1. prepare   one thread per point: transform point and covariance exactly as Open3D does (no FMA
//                contraction, same evaluation order), voxel key, find-or-CLAIM the voxel's slot
//                (claims race through a CAS; same-key racers spin on the LOCKED word until the winner,
//                which finishes its critical section inside the same loop iteration, publishes FULL)
//   2. sort      stable sort of (slot, point index) by slot (vgicp_sort.h, the library's one sort): the points of
//                one voxel become one segment, still in scan order
//   3. apply     the thread at the head of a segment walks it and applies the constructor / addPoint
//                arithmetic of the reference sequentially, in registers, one record write at the end
// Arithmetic is bit-exact with the CPU path (tests compare means, covariances and counts with `==`).
//
// A scan that the device has down-sampled itself (vgicp_scan_prepare: one point per voxel of its grid) puts only a
// handful of points into any voxel of the map, and for those the sort is most of the insertion's time (five launches
// for 27 000 pairs).  launch_map_insert(..., short_lists = true) keeps the order without it:
//   1. prepare   as above, and every point pushes itself onto its voxel's list (the record's spare word is the head:
//                atomic exchange, the old head becomes the point's `next`); the point that found the list empty is the
//                voxel's LEADER
//   2. apply     the leader walks the list, takes the points in ascending index = scan order (a register buffer of
//                kListChunk indices per walk; longer lists take several walks: correct for any length, quadratic
//                beyond the buffer, which is why arbitrary scans keep the sort), applies them, empties the list.
//
// With the raw-point store on (RawLog, VGICP_OPTION_MAP_RAW_POINTS) both apply kernels also keep the points they accept:
// a segment head / list leader knows how many that is before it applies them (min(points, max - count)), reserves as
// many log entries with one add per wave and writes them in its walk — a point's ordinal is the count before it, so the
// export can place every point without ordering the log.  The log is never written past its capacity: the host keeps
// an upper bound of what is appended (every point of an insertion may be accepted) and grows the log before it could
// fill; should an append not fit anyway, ctr[1] is set, nothing is written and the call fails.
//
// Free-space carving (include/vgicp_hip_map_carve.h) takes voxels back: carve_mark_kernel walks a ray per point through
// the table and leaves hits and a shield bit in the low half of the records' spare word (the list head above, zero
// between insertions), carve_sweep_kernel turns the voxels enough rays crossed into tombstones as evict_kernel does and
// clears the marks.  Two launches, nothing in them waits.
//
// The ray report (include/vgicp_hip_map_rays.h) is the read-only query made of the same step: rays_confirm_kernel sets a
// bit per slot that holds a return (a bitmap beside the table, not the spare word), rays_walk_kernel walks every ray up
// to its first FULL voxel and classes it, for several poses in one grid.
//
// Submap as scan (include/vgicp_hip_map_submap.h) makes a resident scan of the table's voxels: eviction's distance test,
// the insertion's transform, and a compaction by ballots and a prefix sum that keeps the slots' order.  Three launches.
//
// The map checkpoint (include/vgicp_hip_map_checkpoint.h) packs the table into a blob with the same three launches and two
// ballots per word (FULL, TOMB), and the restore scatters a blob back slot for slot.
//
// Map merge (include/vgicp_hip_map_merge.h) folds the selected voxels of one table into another, weighted by their
// counts: the submap's MARK and SCAN, a move-and-claim launch that shares the insertion's claim loop (claim_slot), the
// insertion's sort of (slot, rank) and an apply launch that folds a voxel's contributors in the source's slot order.
#include "vgicp_device.h"
#include "vgicp_device_fn.h"
#include "vgicp_sort.h"
#include "vgicp_submap_plan.h"
#include "vgicp_checkpoint_plan.h"
#include "vgicp_merge_plan.h"

namespace vgicp {
namespace {

// table full: after every slot (2^31 slots of 128 B are already 256 GiB), and not 0xFFFFFFFF, the key the sort pads
// with and keeps every key below (vgicp_sort.h)
constexpr uint32_t kNoSlot = 0xFFFFFFFEu;

// C <- R C R^T evaluated as Eigen evaluates (R * C) * R^T: left to right, every product and sum
// rounded once.
__device__ __forceinline__ void rotate_cov_exact(const double* R, const double* C, double* out) {
#pragma clang fp contract(off)
  double RC[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      RC[r + 3 * c] = (R[r] * C[3 * c] + R[r + 3] * C[1 + 3 * c]) + R[r + 6] * C[2 + 3 * c];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      out[r + 3 * c] = (RC[r] * R[c] + RC[r + 3] * R[c + 3]) + RC[r + 6] * R[c + 6];
}

struct InsertScratch {
  double* wpts;        // n x 3 world points
  double* wcovs;       // n x 9 world covariances
  uint32_t* slot_in;   // n
  uint32_t* slot_out;  // n (sorted)
  uint32_t* idx_in;    // n
  uint32_t* idx_out;   // n (sorted)
  void* split;         // the sort's splitters: sortk::split_bytes(n, 4)
};

__host__ inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

__host__ inline InsertScratch carve(void* base, uint32_t n) {
  char* p = static_cast<char*>(base);
  InsertScratch s;
  s.wpts = reinterpret_cast<double*>(p); p += align256((size_t)n * 3 * sizeof(double));
  s.wcovs = reinterpret_cast<double*>(p); p += align256((size_t)n * 9 * sizeof(double));
  s.slot_in = reinterpret_cast<uint32_t*>(p); p += align256((size_t)n * sizeof(uint32_t));
  s.slot_out = reinterpret_cast<uint32_t*>(p); p += align256((size_t)n * sizeof(uint32_t));
  s.idx_in = reinterpret_cast<uint32_t*>(p); p += align256((size_t)n * sizeof(uint32_t));
  s.idx_out = reinterpret_cast<uint32_t*>(p); p += align256((size_t)n * sizeof(uint32_t));
  s.split = p;
  return s;
}

struct Pose12 {
  double v[12];
};

// THE bounded claim loop, the insertion's and the merge's: the slot of the voxel with this key, found or claimed.  fresh:
// this thread created the voxel; returns the slot or kNoSlot (table full).
__device__ __forceinline__ uint32_t claim_slot(VoxelRecord* table, uint32_t mask, int32_t kx, int32_t ky, int32_t kz, bool& fresh) {
  uint32_t slot = voxel_hash(kx, ky, kz) & mask;
  uint32_t found = kNoSlot;
  // `spins` bounds the waits on LOCKED words so that a bug can only fail the call, never hang the GPU
  for (uint32_t probes = 0, spins = 0; probes <= mask && spins < (1u << 22); ++spins) {
    VoxelRecord* rec = table + slot;
    int32_t state = __hip_atomic_load(&rec->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (state == SLOT_EMPTY) {
      int32_t expected = SLOT_EMPTY;
      if (__hip_atomic_compare_exchange_strong(&rec->state, &expected, SLOT_LOCKED, __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        // new voxel: key now, statistics in the apply pass (count 0 marks "not constructed yet")
        rec->key[0] = kx; rec->key[1] = ky; rec->key[2] = kz;
        rec->count = 0;
        rec->reserved = 0;
        __hip_atomic_store(&rec->state, SLOT_FULL, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        fresh = true;
        found = slot;
        break;
      }
      continue;  // lost the race: look at the same slot again
    }
    if (state == SLOT_LOCKED) continue;  // a claim in flight (perhaps of this very key): wait for it
    if (state == SLOT_FULL) {
      // keys are written before FULL is released; read them through the L2 (another CU may own them)
      const int32_t a = __hip_atomic_load(&rec->key[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int32_t b = __hip_atomic_load(&rec->key[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int32_t c = __hip_atomic_load(&rec->key[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a == kx && b == ky && c == kz) { found = slot; break; }
    }
    slot = (slot + 1) & mask;  // other key or tombstone
    ++probes;
  }
  return found;
}

// One point of insert_prepare_kernel: transform, key, find-or-claim the slot. fresh: this thread created the
// voxel; returns the slot or kNoSlot (table full).
__device__ __forceinline__ uint32_t prepare_point(VoxelRecord* table, uint32_t mask, double voxel_size,
                                                  const double* __restrict__ pts, const double* __restrict__ covs,
                                                  uint32_t i, const Pose12& pose, double* __restrict__ wpts,
                                                  double* __restrict__ wcovs, bool& fresh) {
  double p[3], C[9], W[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) C[k] = covs[9 * (size_t)i + k];
  transform_point(pose.v, pose.v + 9, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], p);
  rotate_cov_exact(pose.v, C, W);
#pragma unroll
  for (int k = 0; k < 3; ++k) wpts[3 * (size_t)i + k] = p[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) wcovs[9 * (size_t)i + k] = W[k];
  const int32_t kx = voxel_coord(p[0], voxel_size);
  const int32_t ky = voxel_coord(p[1], voxel_size);
  const int32_t kz = voxel_coord(p[2], voxel_size);
  return claim_slot(table, mask, kx, ky, kz, fresh);
}

// LISTS: idx_of receives the point's `next` on its voxel's list (index + 1 of the point that headed the list before;
// 0: this point found the list empty and is the voxel's leader) instead of the point's own index for the sort.
// keep (may be nullptr): a point whose byte is 0 was refused by a gated insertion's decision (gate_decide_kernel, an
// EARLIER launch): it probes nothing and claims nothing, is not "lost" (counters[1] stays "table full"), and takes
// kNoSlot — behind every real slot in the sort, never the head of a segment — or, LISTS, stands on no list.
template <bool LISTS>
__global__ void insert_prepare_kernel(VoxelRecord* table, uint32_t mask, double voxel_size,
                                      const double* __restrict__ pts, const double* __restrict__ covs,
                                      uint32_t n, Pose12 pose, double* __restrict__ wpts,
                                      double* __restrict__ wcovs, uint32_t* __restrict__ slot_of,
                                      uint32_t* __restrict__ idx_of, uint32_t* counters,
                                      const uint8_t* __restrict__ keep) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool fresh = false, lost = false;
  if (i < n) {
    const bool refused = keep != nullptr && keep[i] == 0;
    const uint32_t found = refused ? kNoSlot : prepare_point(table, mask, voxel_size, pts, covs, i, pose, wpts, wcovs, fresh);
    lost = !refused && found == kNoSlot;
    slot_of[i] = found;
    if constexpr (LISTS) {
      uint32_t next = 0xFFFFFFFFu;  // on no list
      if (found != kNoSlot) next = atomicExch(reinterpret_cast<uint32_t*>(&table[found].reserved), i + 1u);
      idx_of[i] = next;
    } else {
      idx_of[i] = i;
    }
  }
  // one atomic per workgroup and counter (every wave of a scan that opens new ground creates some voxel: one
  // atomic per wave on the same word was half of this kernel's time)
  const int created = __syncthreads_count(fresh ? 1 : 0);
  const int failed = __syncthreads_count(lost ? 1 : 0);
  if (threadIdx.x == 0) {
    if (created) atomicAdd(&counters[0], (uint32_t)created);
    if (failed) atomicAdd(&counters[1], (uint32_t)failed);
  }
}

// Raw-point store: base of `k` consecutive log entries for this lane (block_reserve below).
// Points of `len` that the constructor / addPoint accept into a voxel that holds `count` (max_points >= 1).
__device__ __forceinline__ uint32_t accepted_points(uint64_t count, uint32_t len, uint64_t max_points) {
  const uint64_t room = count < max_points ? max_points - count : 0;
  return (uint64_t)len < room ? len : (uint32_t)room;
}

// The same for the whole workgroup (kBlock threads, every one of them here): one atomic per workgroup — the
// insertion's kernels are short, and hundreds of waves adding to one word cost more than the scan.
constexpr uint32_t kBlock = 256;
__device__ __forceinline__ uint32_t block_reserve(uint32_t* counter, uint32_t k) {
  __shared__ uint32_t wave_total[kBlock / 64];
  __shared__ uint32_t block_base;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = k;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(incl, (unsigned int)d, 64);
    if ((int)lane >= d) incl += v;
  }
  if (lane == 63u) wave_total[wave] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kBlock / 64; ++w) {
    before += w < wave ? wave_total[w] : 0u;
    total += wave_total[w];
  }
  if (threadIdx.x == 0) block_base = total ? atomicAdd(counter, total) : 0u;
  __syncthreads();
  return block_base + before + incl - k;
}

// The log entries of one segment / list: reserved by every lane of the workgroup, `k` of them for this lane; false
// (and ctr[1] set) when they do not fit.
__device__ __forceinline__ bool raw_reserve(const RawLog& raw, uint32_t k, uint32_t& at) {
  at = block_reserve(&raw.ctr[0], k);
  const bool fits = (uint64_t)at + k <= raw.capacity;
  if (k != 0u && !fits) atomicOr(&raw.ctr[1], 1u);
  return fits;
}

__device__ __forceinline__ void raw_write(const RawLog& raw, uint32_t at, const double* __restrict__ wpts, uint32_t i,
                                          uint32_t slot, uint64_t ordinal) {
  RawPoint* e = raw.entries + at;
#pragma unroll
  for (int k = 0; k < 3; ++k) e->xyz[k] = wpts[3 * (size_t)i + k];
  e->slot = slot;
  e->ordinal = (uint32_t)ordinal;
}

// Voxel(max, p, C) / Voxel::addPoint applied to the segment that starts at sorted position j.
template <bool RAW>
__global__ void insert_apply_kernel(VoxelRecord* table, const uint32_t* __restrict__ slot_sorted,
                                    const uint32_t* __restrict__ idx_sorted, uint32_t n,
                                    const double* __restrict__ wpts, const double* __restrict__ wcovs,
                                    uint64_t max_points, RawLog raw) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t slot = kNoSlot;
  bool head = false;
  if (j < n) {
    slot = slot_sorted[j];
    head = slot != kNoSlot && !(j > 0 && slot_sorted[j - 1] == slot);  // the head of its segment
  }
  uint32_t at = 0;
  bool keep = false;
  if constexpr (RAW) {
    uint32_t len = 0;
    if (head)
      for (uint32_t q = j; q < n && slot_sorted[q] == slot; ++q) ++len;
    keep = raw_reserve(raw, head ? accepted_points(table[slot].count, len, max_points) : 0u, at);
  }
  if (!head) return;
  VoxelRecord* rec = table + slot;
  uint64_t count = rec->count;
  double mean[3], cov[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) mean[k] = rec->mean[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) cov[k] = rec->cov[k];
  for (uint32_t q = j; q < n && slot_sorted[q] == slot; ++q) {
    const uint32_t i = idx_sorted[q];
    if (count == 0) {  // constructor
      if constexpr (RAW) { if (keep) raw_write(raw, at++, wpts, i, slot, count); }
#pragma unroll
      for (int k = 0; k < 3; ++k) mean[k] = wpts[3 * (size_t)i + k];
#pragma unroll
      for (int k = 0; k < 9; ++k) cov[k] = wcovs[9 * (size_t)i + k];
      count = 1;
    } else if (count < max_points) {  // addPoint
#pragma clang fp contract(off)
      const double nn = (double)count, n1 = (double)(count + 1);
#pragma unroll
      for (int k = 0; k < 3; ++k) mean[k] = (nn * mean[k] + wpts[3 * (size_t)i + k]) / n1;
#pragma unroll
      for (int k = 0; k < 9; ++k) cov[k] = (nn * cov[k] + wcovs[9 * (size_t)i + k]) / n1;
      if constexpr (RAW) { if (keep) raw_write(raw, at++, wpts, i, slot, count); }
      ++count;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) rec->mean[k] = mean[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) rec->cov[k] = cov[k];
  rec->count = count;
}

// The same for a voxel whose points hang on its list (short_lists): run by the voxel's leader.
constexpr int kListChunk = 8;
template <bool RAW>
__global__ void insert_apply_list_kernel(VoxelRecord* table, const uint32_t* __restrict__ slot_of,
                                         const uint32_t* __restrict__ next_of, uint32_t n,
                                         const double* __restrict__ wpts, const double* __restrict__ wcovs,
                                         uint64_t max_points, RawLog raw) {
  const uint32_t me = blockIdx.x * blockDim.x + threadIdx.x;
  const bool leader = me < n && next_of[me] == 0u;  // not: on no list (table full), or not the leader
  if (!RAW && !leader) return;                        // (the store's reservation needs every lane of the workgroup)
  const uint32_t slot = leader ? slot_of[me] : 0u;
  VoxelRecord* rec = table + slot;
  uint32_t head = 0;  // index + 1 of the point that pushed itself last
  uint64_t count = 0;
  double mean[3], cov[9];
  if (leader) {
    head = (uint32_t)rec->reserved;
    count = rec->count;
#pragma unroll
    for (int k = 0; k < 3; ++k) mean[k] = rec->mean[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) cov[k] = rec->cov[k];
  }
  uint32_t at = 0;
  bool keep = false;
  auto apply = [&](uint32_t i) {
    if (count == 0) {  // constructor
      if constexpr (RAW) { if (keep) raw_write(raw, at++, wpts, i, slot, count); }
#pragma unroll
      for (int k = 0; k < 3; ++k) mean[k] = wpts[3 * (size_t)i + k];
#pragma unroll
      for (int k = 0; k < 9; ++k) cov[k] = wcovs[9 * (size_t)i + k];
      count = 1;
    } else if (count < max_points) {  // addPoint
#pragma clang fp contract(off)
      const double nn = (double)count, n1 = (double)(count + 1);
#pragma unroll
      for (int k = 0; k < 3; ++k) mean[k] = (nn * mean[k] + wpts[3 * (size_t)i + k]) / n1;
#pragma unroll
      for (int k = 0; k < 9; ++k) cov[k] = (nn * cov[k] + wcovs[9 * (size_t)i + k]) / n1;
      if constexpr (RAW) { if (keep) raw_write(raw, at++, wpts, i, slot, count); }
      ++count;
    }
  };
  // ascending index, kListChunk at a time: every walk keeps the smallest indices above the last one applied
  uint32_t buf[kListChunk];
  auto gather = [&](long long after) {
#pragma unroll
    for (int k = 0; k < kListChunk; ++k) buf[k] = 0xFFFFFFFFu;
    int held = 0;
    for (uint32_t cur = head; cur != 0u; cur = next_of[cur - 1u]) {
      uint32_t x = cur - 1u;
      if ((long long)x <= after) continue;
      // insert x into the ascending buffer, dropping the largest when it is full (static indices: registers)
#pragma unroll
      for (int k = 0; k < kListChunk; ++k) {
        const uint32_t lo = x < buf[k] ? x : buf[k], hi = x < buf[k] ? buf[k] : x;
        buf[k] = lo;
        x = hi;
      }
      if (held < kListChunk) ++held;
    }
    return held;
  };
  int held = 0;
  if (leader) {
    if (head == me + 1u) {  // the usual case: the voxel received this one point
      buf[0] = me;
      held = 1;
    } else {
      held = gather(-1);
    }
  }
  if constexpr (RAW) {
    // the list's length: the first walk has it unless the list is longer than one chunk
    uint32_t len = (uint32_t)held;
    if (held == kListChunk) {
      len = 0;
      for (uint32_t cur = head; cur != 0u; cur = next_of[cur - 1u]) ++len;
    }
    keep = raw_reserve(raw, leader ? accepted_points(count, len, max_points) : 0u, at);
    if (!leader) return;
  }
  long long done = -1;  // the largest index applied so far
  for (;;) {
#pragma unroll
    for (int k = 0; k < kListChunk; ++k)
      if (k < held) { apply(buf[k]); done = (long long)buf[k]; }
    if (held < kListChunk) break;
    held = gather(done);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) rec->mean[k] = mean[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) rec->cov[k] = cov[k];
  rec->count = count;
  rec->reserved = 0;  // the list is empty again
}

// LocalMap::needsPointRemoval (voxel_beyond, vgicp_device_fn.h: the submap's selection asks the same question)
__global__ void evict_kernel(VoxelRecord* table, uint64_t slots, double voxel_size, double px,
                             double py, double pz, double distance, uint32_t* counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool far = false;
  if (i < slots && table[i].state == SLOT_FULL) {
    VoxelRecord* rec = table + i;
    far = voxel_beyond(rec->key[0], rec->key[1], rec->key[2], voxel_size, px, py, pz, distance);
    if (far) rec->state = SLOT_TOMB;
  }
  // one atomic per workgroup: a mass eviction (788k of 1M voxels) was bound by 16 000 waves adding to one word
  const int gone = __syncthreads_count(far ? 1 : 0);
  if (threadIdx.x == 0 && gone) atomicAdd(&counters[0], (uint32_t)gone);
}

// ---- free-space carving (include/vgicp_hip_map_carve.h states the rule operation by operation; this restates it) ----
// (carve_key, the key that is DEFINED within +-2^30, is vgicp_device_fn.h's: vgicp_levels.hip's locate reads it too)
// The voxel with this key, if it is FULL, takes `mark` into the low half of its spare word (no value comes back).  The
// probe is find_voxel's: one 16-byte access per slot (key + state), linear, stops at EMPTY, skips TOMB and other keys.
__device__ __forceinline__ void carve_mark(VoxelRecord* table, uint32_t mask, int32_t kx, int32_t ky, int32_t kz, bool shield) {
  const VoxelRecord* rec = find_voxel(table, mask, kx, ky, kz);
  if (!rec) return;
  uint32_t* word = reinterpret_cast<uint32_t*>(&const_cast<VoxelRecord*>(rec)->reserved);
  if (!shield) {
    atomicAdd(word, 1u);
  } else if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kCarveShield)) {
    atomicOr(word, kCarveShield);   // (a scan puts many points into one voxel: most find the bit set)
  }
}
// the parameter at which the ray leaves voxel k along one axis
__device__ __forceinline__ double carve_boundary(int32_t k, double d, double o, double h) {
#pragma clang fp contract(off)
  if (d == 0.0) return __builtin_inf();
  return ((double)(k + (d > 0.0 ? 1 : 0)) * h - o) / d;
}
// THE walk of a ray through the voxels, carving's and the ray report's: from the voxel of the origin o (key k0) along d
// (len: its length) while the parameter of the next boundary is below t_end.  visit(kx, ky, kz) is called for the
// origin's voxel and for every voxel entered; true stops the walk.  What comes back: the voxels visited, the last one's
// key and the parameter at which the ray entered it (0 in the origin's).
struct RayWalk {
  uint32_t visits;
  int32_t kx, ky, kz;
  double t_in;
};
template <class Visit>
__device__ __forceinline__ RayWalk walk_ray(const int32_t* k0, double dx, double dy, double dz, const double* o, double h,
                                            double t_end, double len, Visit visit) {
#pragma clang fp contract(off)
  // the walk's hard bound: what vgicp_map_plan.h lets through keeps the ceiling at kCarveMaxSteps + 1
  constexpr double kCellsMax = 4097.0;
  double cells = ceil((t_end * len) / h);
  if (!(cells <= kCellsMax)) cells = kCellsMax;   // (a NaN too)
  const uint32_t max_steps = 3u * (uint32_t)cells + 3u;
  RayWalk w{1u, k0[0], k0[1], k0[2], 0.0};
  const int32_t sx = dx > 0.0 ? 1 : -1, sy = dy > 0.0 ? 1 : -1, sz = dz > 0.0 ? 1 : -1;
  double tx = carve_boundary(w.kx, dx, o[0], h), ty = carve_boundary(w.ky, dy, o[1], h), tz = carve_boundary(w.kz, dz, o[2], h);
  bool stop = visit(w.kx, w.ky, w.kz);
  for (uint32_t step = 0; step < max_steps && !stop; ++step) {
    if (tx <= ty && tx <= tz) {
      if (!(tx < t_end)) break;
      w.t_in = tx;
      w.kx += sx;
      tx = carve_boundary(w.kx, dx, o[0], h);
    } else if (ty <= tz) {
      if (!(ty < t_end)) break;
      w.t_in = ty;
      w.ky += sy;
      ty = carve_boundary(w.ky, dy, o[1], h);
    } else {
      if (!(tz < t_end)) break;
      w.t_in = tz;
      w.kz += sz;
      tz = carve_boundary(w.kz, dz, o[2], h);
    }
    stop = visit(w.kx, w.ky, w.kz);
    ++w.visits;
  }
  return w;
}
// The workgroup's 64-bit sum of every lane's `visits`, for thread 0 (every thread of a kBlock workgroup calls this).
__device__ __forceinline__ unsigned long long block_visits(uint32_t visits) {
  __shared__ unsigned long long wave_visits[kBlock / 64];
  unsigned long long sum = visits;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, (unsigned int)d, 64);
  if ((threadIdx.x & 63u) == 0u) wave_visits[threadIdx.x >> 6] = sum;
  __syncthreads();
  unsigned long long total = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) total += wave_visits[w];
  }
  return total;
}

__global__ void __launch_bounds__(kBlock) carve_mark_kernel(CarveArgs a) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t mask = (uint32_t)(a.slots - 1);
  const double h = a.voxel_size;
  bool ray = false;
  uint32_t visits = 0;
  if (i < a.n) {
    double e[3];
    int32_t k[3];
    transform_point(a.pose, a.pose + 9, a.points_aos[3 * (size_t)i], a.points_aos[3 * (size_t)i + 1], a.points_aos[3 * (size_t)i + 2], e);
    if (carve_key(e, h, k)) carve_mark(a.table, mask, k[0], k[1], k[2], /*shield=*/true);
    if (i % a.stride == 0u) {
      double o[3];
      transform_point(a.pose, a.pose + 9, a.origin[0], a.origin[1], a.origin[2], o);
      const double dx = e[0] - o[0], dy = e[1] - o[1], dz = e[2] - o[2];
      const double len = sqrt((dx * dx + dy * dy) + dz * dz);
      const double shorter = len - a.margin;
      const double t_stop = (shorter < a.max_range ? shorter : a.max_range) / len;
      const bool finite = isfinite(dx) && isfinite(dy) && isfinite(dz);
      if (t_stop > 0.0 && finite && carve_key(o, h, k)) {
        ray = true;
        visits = walk_ray(k, dx, dy, dz, o, h, t_stop, len, [&](int32_t kx, int32_t ky, int32_t kz) {
                   carve_mark(a.table, mask, kx, ky, kz, false);
                   return false;   // carving marks every voxel up to t_stop
                 }).visits;
      }
    }
  }
  // one atomic per workgroup and counter
  const int cast = __syncthreads_count(ray ? 1 : 0);
  const unsigned long long total = block_visits(visits);
  if (threadIdx.x == 0) {
    if (a.rays && cast) atomicAdd(a.rays, (uint32_t)cast);
    if (a.visits && total) atomicAdd(a.visits, total);
  }
}

// One lane per slot, as evict_kernel: a slot whose marks are not zero is decided and its marks cleared.
__global__ void __launch_bounds__(kBlock) carve_sweep_kernel(CarveArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool touched = false, shielded = false, gone = false;
  VoxelRecord* rec = a.table + (i < a.slots ? i : 0);
  if (i < a.slots) {
    uint32_t* word = reinterpret_cast<uint32_t*>(&rec->reserved);
    const uint32_t marks = *word;
    if (marks != 0u) {
      *word = 0u;
      if (rec->state == SLOT_FULL) {   // (marks land on FULL records only)
        const uint32_t hits = marks & ~kCarveShield;
        touched = hits >= 1u;
        shielded = touched && (marks & kCarveShield) != 0u;
        gone = hits >= a.min_hits && (marks & kCarveShield) == 0u;
        if (gone) rec->state = SLOT_TOMB;
      }
    }
  }
  const int n_touched = __syncthreads_count(touched ? 1 : 0);
  const int n_shielded = __syncthreads_count(shielded ? 1 : 0);
  if (threadIdx.x == 0) {
    if (a.touched && n_touched) atomicAdd(a.touched, (uint32_t)n_touched);
    if (a.shielded && n_shielded) atomicAdd(a.shielded, (uint32_t)n_shielded);
  }
  // the count and, when a key list is wanted, every removed voxel's place in it: one atomic per workgroup
  const uint32_t pos = block_reserve(a.removed, gone ? 1u : 0u);
  if (gone && a.keys && pos < a.keys_capacity) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.keys[3 * (size_t)pos + k] = rec->key[k];
  }
}

// ---- the ray report (include/vgicp_hip_map_rays.h states the rule operation by operation; this restates it).  The key,
// the boundary, the walk (walk_ray), the transform and the probe are carving's above: one definition serves both ----
// CONFIRM: one lane per point and pose.  The slot of the point's own voxel, if FULL, gets its bit in the pose's bitmap
// (test before set, as carve_mark does for the shield: a scan puts many points into one voxel).
__global__ void __launch_bounds__(kBlock) rays_confirm_kernel(RayArgs a) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const double* pose = a.poses + 12 * (size_t)blockIdx.y;
  uint32_t* bits = a.bits + (size_t)blockIdx.y * (size_t)(a.slots >> 5);
  double e[3];
  int32_t k[3];
  transform_point(pose, pose + 9, a.points_aos[3 * (size_t)i], a.points_aos[3 * (size_t)i + 1], a.points_aos[3 * (size_t)i + 2], e);
  if (!carve_key(e, a.voxel_size, k)) return;
  const VoxelRecord* rec = find_voxel(a.table, (uint32_t)(a.slots - 1), k[0], k[1], k[2]);
  if (!rec) return;
  const uint64_t slot = (uint64_t)(rec - a.table);
  uint32_t* word = bits + (slot >> 5);
  const uint32_t bit = 1u << (slot & 31u);
  if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
}

// WALK: one lane per point and pose.  The ray's walk up to the first FULL voxel, the class, the planes, the counts.
__global__ void __launch_bounds__(kBlock) rays_walk_kernel(RayArgs a) {
#pragma clang fp contract(off)
  __shared__ uint32_t by_class[8];
  if (threadIdx.x < 8u) by_class[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t mask = (uint32_t)(a.slots - 1);
  const double h = a.voxel_size;
  const double* pose = a.poses + 12 * (size_t)blockIdx.y;
  const uint32_t* bits = a.bits + (size_t)blockIdx.y * (size_t)(a.slots >> 5);
  bool ray = false;
  uint32_t visits = 0;
  if (i < a.n) {
    uint32_t cls = 0u;   // NO_RAY
    const VoxelRecord* hit = nullptr;
    double t_in = 0.0, len = 0.0;
    int32_t kx = 0, ky = 0, kz = 0;
    double e[3];
    if (i % a.stride == 0u) {
      double o[3];
      int32_t k[3];
      transform_point(pose, pose + 9, a.points_aos[3 * (size_t)i], a.points_aos[3 * (size_t)i + 1], a.points_aos[3 * (size_t)i + 2], e);
      transform_point(pose, pose + 9, a.origin[0], a.origin[1], a.origin[2], o);
      const double dx = e[0] - o[0], dy = e[1] - o[1], dz = e[2] - o[2];
      len = sqrt((dx * dx + dy * dy) + dz * dz);
      const double longer = len + a.beyond;
      const double t_end = (longer < a.max_range ? longer : a.max_range) / len;
      const double t_front = (len - a.margin) / len;
      const bool finite = isfinite(dx) && isfinite(dy) && isfinite(dz);
      if (len > 0.0 && t_end > 0.0 && finite && carve_key(o, h, k)) {
        ray = true;
        const RayWalk w = walk_ray(k, dx, dy, dz, o, h, t_end, len, [&](int32_t x, int32_t y, int32_t z) {
          hit = find_voxel(a.table, mask, x, y, z);
          return hit != nullptr;   // the report ends at the first FULL voxel
        });
        visits = w.visits;
        kx = w.kx; ky = w.ky; kz = w.kz;
        t_in = w.t_in;
        // the class, in the header's order
        if (!hit) {
          cls = 1u;   // OPEN
        } else {
          int32_t ke[3];
          const bool own = carve_key(e, h, ke) && ke[0] == kx && ke[1] == ky && ke[2] == kz;
          const uint64_t slot = (uint64_t)(hit - a.table);
          const bool confirmed = (bits[slot >> 5] >> (slot & 31u)) & 1u;
          cls = own ? 2u : t_in >= 1.0 ? 3u : confirmed ? 4u : t_in < t_front ? 5u : 6u;
        }
      }
    }
    atomicAdd(&by_class[cls], 1u);
    if (a.status) a.status[i] = (uint8_t)cls;
    if (a.range) a.range[i] = hit ? t_in * len : __longlong_as_double(0x7FF8000000000000ll);
    if (a.hit_key) {
      a.hit_key[3 * (size_t)i] = hit ? kx : INT32_MIN;
      a.hit_key[3 * (size_t)i + 1] = hit ? ky : INT32_MIN;
      a.hit_key[3 * (size_t)i + 2] = hit ? kz : INT32_MIN;
    }
    if (a.steps) a.steps[i] = visits;
  }
  // at most one global atomic per workgroup and counter
  const int cast = __syncthreads_count(ray ? 1 : 0);   // (also the barrier behind the histogram's adds)
  const unsigned long long total = block_visits(visits);
  unsigned long long* counts = a.counts + (size_t)kRayCountWords * blockIdx.y;
  if (threadIdx.x == 0) {
    if (cast) atomicAdd(counts, (unsigned long long)cast);
    if (total) atomicAdd(counts + 1, total);
  }
  if (threadIdx.x < 8u && by_class[threadIdx.x]) atomicAdd(counts + 2 + threadIdx.x, (unsigned long long)by_class[threadIdx.x]);
}

__global__ void export_kernel(const VoxelRecord* __restrict__ table, uint64_t slots, uint32_t capacity,
                              int32_t* __restrict__ keys, double* __restrict__ means,
                              double* __restrict__ covs, uint64_t* __restrict__ counts,
                              uint32_t* counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slots) return;
  const VoxelRecord* rec = table + i;
  if (rec->state != SLOT_FULL) return;
  const uint32_t pos = wave_append(&counters[0]);
  if (pos >= capacity) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    keys[3 * (size_t)pos + k] = rec->key[k];
    means[3 * (size_t)pos + k] = rec->mean[k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) covs[9 * (size_t)pos + k] = rec->cov[k];
  counts[pos] = rec->count;
}

// ---- the raw-point store (RawLog) ----
// An entry's slot is checked against the table before it is used: after an append that did not fit (ctr[1]; the call
// that made it failed) the log may hold entries nobody wrote, and those must not index anything.
__global__ void raw_compact_kernel(const RawPoint* __restrict__ src, uint32_t src_upper, const uint32_t* ctr,
                                   const VoxelRecord* __restrict__ table, uint64_t slots,
                                   const uint32_t* __restrict__ claimed, RawPoint* __restrict__ dst,
                                   uint32_t dst_capacity, uint32_t* dst_ctr) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t used = ctr[0] < src_upper ? ctr[0] : src_upper;
  if (e >= used) return;
  RawPoint p = src[e];
  if ((uint64_t)p.slot >= slots) return;
  if (claimed) {
    const uint32_t c = claimed[p.slot];
    if (c == kClaimFailed) return;  // the voxel was gone before the rehash
    p.slot = c & ~kClaimFresh;
  } else if (table[p.slot].state != SLOT_FULL) {
    return;
  }
  const uint32_t pos = wave_append(dst_ctr);
  if (pos < dst_capacity) dst[pos] = p;
}

__global__ void raw_offsets_kernel(const VoxelRecord* __restrict__ table, uint64_t slots, uint32_t* __restrict__ offsets,
                                   uint32_t* total) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t c = 0;
  if (i < slots && table[i].state == SLOT_FULL) c = (uint32_t)table[i].count;
  const uint32_t at = block_reserve(total, c);
  if (offsets && i < slots) offsets[i] = at;
}

__global__ void raw_scatter_kernel(const RawPoint* __restrict__ log, uint32_t upper, const uint32_t* ctr,
                                   const VoxelRecord* __restrict__ table, uint64_t slots,
                                   const uint32_t* __restrict__ offsets, uint32_t capacity, int32_t* __restrict__ keys,
                                   double* __restrict__ points) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t used = ctr[0] < upper ? ctr[0] : upper;
  if (e >= used) return;
  const RawPoint p = log[e];
  if ((uint64_t)p.slot >= slots) return;   // see raw_compact_kernel
  const VoxelRecord* rec = table + p.slot;
  if (rec->state != SLOT_FULL || p.ordinal >= rec->count) return;  // dead (evicted / erased voxel)
  const uint64_t pos = (uint64_t)offsets[p.slot] + p.ordinal;
  if (pos >= capacity) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    keys[3 * pos + k] = rec->key[k];
    points[3 * pos + k] = p.xyz[k];
  }
}

// ---- submap as scan (include/vgicp_hip_map_submap.h states the rule operation by operation; this restates it) ----
// MARK.  As the levels' claim launch: a thread issues the loads of its kSubmapPer slot heads together (one 16-byte read
// out of every 128-byte line of a mostly EMPTY table; what it costs is how many are in flight).  Turn k of wave w covers
// the 64 consecutive slots of ballot word k * 4 + w of the group.
__global__ __launch_bounds__(kSubmapBlock) void submap_mark_kernel(SubmapArgs a) {
  __shared__ uint32_t sums[3];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid < 3u) sums[tid] = 0u;
  __syncthreads();
  const uint64_t first_slot = (uint64_t)blockIdx.x * kSubmapGroupSlots + tid;
  int4 heads[kSubmapPer];
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k) {
    const uint64_t i = first_slot + kSubmapBlock * k;
    heads[k] = i < a.slots ? *reinterpret_cast<const int4*>(a.table + i) : make_int4(0, 0, 0, SLOT_EMPTY);
  }
  uint32_t taken = 0, far = 0, few = 0;   // lane 0's: the wave's counts
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k) {
    const int4 head = heads[k];
    const bool full = head.w == SLOT_FULL;
    const bool beyond = full && voxel_beyond(head.x, head.y, head.z, a.voxel_size, a.center[0], a.center[1], a.center[2], a.radius);
    const bool inside = full && !beyond;
    bool enough = true;
    if (inside && a.min_count > 1ull) enough = a.table[first_slot + kSubmapBlock * k].count >= a.min_count;
    const unsigned long long ballot = __ballot(inside && enough);
    const unsigned long long b_far = __ballot(beyond), b_few = __ballot(inside && !enough);
    if (lane == 0u) {
      a.ballots[(size_t)blockIdx.x * kSubmapGroupWords + k * (kSubmapBlock / 64u) + wave] = ballot;
      taken += (uint32_t)__popcll(ballot);
      far += (uint32_t)__popcll(b_far);
      few += (uint32_t)__popcll(b_few);
    }
  }
  if (lane == 0u) {   // integers: the order of the four waves does not matter
    if (taken) atomicAdd(&sums[0], taken);
    if (far) atomicAdd(&sums[1], far);
    if (few) atomicAdd(&sums[2], few);
  }
  __syncthreads();
  if (tid < 3u) a.group_counts[(size_t)tid * a.groups + blockIdx.x] = sums[tid];
}

// SCAN.  One workgroup: the exclusive prefix sum of the groups' selected counts in place, 1 024 at a time with a carry,
// and the three totals.
__global__ __launch_bounds__(1024) void submap_scan_kernel(uint32_t* counts, uint32_t groups, unsigned long long* totals,
                                                          unsigned long long* totals_host) {
  __shared__ uint32_t wave_sum[16];
  __shared__ unsigned long long wave_left[2][16];
  __shared__ uint32_t carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0u) carry = 0u;
  __syncthreads();
  unsigned long long far = 0ull, few = 0ull;
  for (uint32_t base = 0; base < groups; base += 1024u) {
    const uint32_t idx = base + tid;
    const uint32_t val = idx < groups ? counts[idx] : 0u;
    if (idx < groups) {
      far += counts[(size_t)groups + idx];
      few += counts[2 * (size_t)groups + idx];
    }
    uint32_t incl = val;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t w = 0; w < wave; ++w) before += wave_sum[w];
    if (idx < groups) counts[idx] = before + incl - val;
    __syncthreads();
    if (tid == 1023u) carry = before + incl;
    __syncthreads();
  }
  for (int d = 32; d > 0; d >>= 1) {
    far += __shfl_down(far, d, 64);
    few += __shfl_down(few, d, 64);
  }
  if (lane == 0u) {
    wave_left[0][wave] = far;
    wave_left[1][wave] = few;
  }
  __syncthreads();
  if (tid != 0u) return;
  for (uint32_t w = 1; w < 16u; ++w) {
    far += wave_left[0][w];
    few += wave_left[1][w];
  }
  const unsigned long long out[3] = {carry, far, few};
  for (int k = 0; k < 3; ++k) totals[k] = totals_host[k] = out[k];
}

// EMIT.  The group's kSubmapGroupWords ballots sit in the first lanes of every wave; their popcounts' prefix gives what
// lies before each word.  A group that selected nothing leaves at once, a zero word touches no table line.
__global__ __launch_bounds__(kSubmapBlock) void submap_emit_kernel(SubmapArgs a) {
  static_assert(kSubmapGroupWords <= 64u, "a wave holds its group's ballots, one per lane");
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned long long mine = lane < kSubmapGroupWords ? a.ballots[(size_t)blockIdx.x * kSubmapGroupWords + lane] : 0ull;
  const uint32_t pc = (uint32_t)__popcll(mine);
  uint32_t incl = pc;
#pragma unroll
  for (int d = 1; d < (int)kSubmapGroupWords; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += up;
  }
  if (__shfl(incl, (int)kSubmapGroupWords - 1, 64) == 0u) return;   // the whole group, so the whole workgroup
  const uint32_t excl = incl - pc;
  const uint32_t base = a.group_counts[blockIdx.x];
  unsigned long long word[kSubmapPer];
  uint32_t before[kSubmapPer];
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k) {   // every lane takes part in the cross-lane reads
    const int q = (int)(k * (kSubmapBlock / 64u) + wave);
    word[k] = __shfl(mine, q, 64);
    before[k] = __shfl(excl, q, 64);
  }
#pragma unroll 1
  for (uint32_t k = 0; k < kSubmapPer; ++k) {
    if (!((word[k] >> lane) & 1ull)) continue;
    const size_t rank = (size_t)base + before[k] + (uint32_t)__popcll(word[k] & ((1ull << lane) - 1ull));
    if (rank >= a.capacity) continue;   // the host sizes the outputs for every voxel of the table; this is the belt
    const VoxelRecord* rec = a.table + ((uint64_t)blockIdx.x * kSubmapGroupSlots + kSubmapBlock * k + tid);
    const int4 head = *reinterpret_cast<const int4*>(rec);
    const double2* pay = reinterpret_cast<const double2*>(rec->mean);   // 16-byte aligned
    const double2 p0 = pay[0], p1 = pay[1], p2 = pay[2], p3 = pay[3], p4 = pay[4], p5 = pay[5];
    const unsigned long long count = rec->count;
    const double C[9] = {p1.y, p2.x, p2.y, p3.x, p3.y, p4.x, p4.y, p5.x, p5.y};
    double v[kScanPlanes];
    transform_point(a.pose, a.pose + 9, p0.x, p0.y, p1.x, v);
    rotate_cov_exact(a.pose, C, v + 3);
#pragma unroll
    for (int e = 0; e < 3; ++e) a.aos_points[3 * rank + e] = v[e];
#pragma unroll
    for (int e = 0; e < 9; ++e) a.aos_covs[9 * rank + e] = v[3 + e];
#pragma unroll
    for (int e = 0; e < kScanPlanes; ++e) a.planes[(size_t)e * a.stride + rank] = v[e];   // consecutive ranks: contiguous
    a.keys[3 * rank] = head.x;
    a.keys[3 * rank + 1] = head.y;
    a.keys[3 * rank + 2] = head.z;
    a.counts[rank] = count;
  }
}

// ---- map checkpoint (include/vgicp_hip_map_checkpoint.h has the format) ----
// MARK.  The submap's, with two ballots per turn and no decision but the state; with raw points the wave also sums its
// FULL records' counts (one 8-byte read out of the line the head came from).
__global__ __launch_bounds__(kSubmapBlock) void checkpoint_mark_kernel(CheckpointArgs a) {
  __shared__ uint32_t sums[3];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid < 3u) sums[tid] = 0u;
  __syncthreads();
  const uint64_t first_slot = (uint64_t)blockIdx.x * kSubmapGroupSlots + tid;
  int4 heads[kSubmapPer];
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k) {
    const uint64_t i = first_slot + kSubmapBlock * k;
    heads[k] = i < a.slots ? *reinterpret_cast<const int4*>(a.table + i) : make_int4(0, 0, 0, SLOT_EMPTY);
  }
  uint32_t n_full = 0, n_tomb = 0, n_raw = 0;   // lane 0's: the wave's counts
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k) {
    const bool full = heads[k].w == SLOT_FULL;
    const unsigned long long b_full = __ballot(full), b_tomb = __ballot(heads[k].w == SLOT_TOMB);
    uint32_t points = 0;
    if (a.word_raw) {   // the same for every lane
      points = full ? (uint32_t)a.table[first_slot + kSubmapBlock * k].count : 0u;
      for (int d = 32; d > 0; d >>= 1) points += __shfl_down(points, d, 64);
    }
    if (lane == 0u) {
      const uint32_t q = k * (kSubmapBlock / 64u) + wave;
      a.ballots[((size_t)blockIdx.x * 2) * kSubmapGroupWords + q] = b_full;
      a.ballots[((size_t)blockIdx.x * 2 + 1) * kSubmapGroupWords + q] = b_tomb;
      if (a.word_raw) a.word_raw[(size_t)blockIdx.x * kSubmapGroupWords + q] = points;
      n_full += (uint32_t)__popcll(b_full);
      n_tomb += (uint32_t)__popcll(b_tomb);
      n_raw += points;
    }
  }
  if (lane == 0u) {   // integers: the order of the four waves does not matter
    if (n_full) atomicAdd(&sums[0], n_full);
    if (n_tomb) atomicAdd(&sums[1], n_tomb);
    if (n_raw) atomicAdd(&sums[2], n_raw);
  }
  __syncthreads();
  if (tid < 3u) a.group_counts[(size_t)tid * a.groups + blockIdx.x] = sums[tid];
}

// SCAN.  One workgroup: the exclusive prefix sum of each of `arrays` rows of `groups` counts in place, 1 024 at a time
// with a carry, and each row's total (to both places; totals_host may be nullptr).
__global__ __launch_bounds__(1024) void checkpoint_scan_kernel(uint32_t* counts, uint32_t groups, uint32_t arrays,
                                                              unsigned long long* totals, unsigned long long* totals_host) {
  __shared__ uint32_t wave_sum[16];
  __shared__ uint32_t carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (uint32_t r = 0; r < arrays; ++r) {
    uint32_t* row = counts + (size_t)r * groups;
    if (tid == 0u) carry = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < groups; base += 1024u) {
      const uint32_t idx = base + tid;
      const uint32_t val = idx < groups ? row[idx] : 0u;
      uint32_t incl = val;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
      }
      if (lane == 63u) wave_sum[wave] = incl;
      __syncthreads();
      uint32_t before = carry;
      for (uint32_t w = 0; w < wave; ++w) before += wave_sum[w];
      if (idx < groups) row[idx] = before + incl - val;
      __syncthreads();
      if (tid == 1023u) carry = before + incl;
      __syncthreads();
    }
    if (tid == 0u) {
      totals[r] = carry;
      if (totals_host) totals_host[r] = carry;
    }
    __syncthreads();
  }
}

// EMIT.  A wave holds its group's ballots and sums, one per lane: lanes 0 .. 15 the FULL words, 16 .. 31 the TOMB words,
// 32 .. 47 the raw sums; a prefix sum inside each run of 16 lanes gives what lies before each word.  A lane's slot and
// rank as in the submap's EMIT; the records are then copied eight lanes to a record, 16 bytes each: every read and every
// write is a whole line.  The last 16 bytes are the count and the spare word, which goes out as zero.
__global__ __launch_bounds__(kSubmapBlock) void checkpoint_emit_kernel(CheckpointArgs a) {
  static_assert(kSubmapGroupWords == 16u, "three runs of 16 lanes hold a group's ballots and sums");
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, seg = lane >> 4, in_seg = lane & 15u;
  const size_t g = blockIdx.x;
  unsigned long long mine = 0ull;
  if (seg < 2u) mine = a.ballots[(g * 2 + seg) * kSubmapGroupWords + in_seg];
  uint32_t val = (uint32_t)__popcll(mine);
  if (seg == 2u && a.word_raw) val = a.word_raw[g * kSubmapGroupWords + in_seg];
  uint32_t incl = val;
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if (in_seg >= (uint32_t)d) incl += up;
  }
  if (__shfl(incl, 15, 64) == 0u && __shfl(incl, 31, 64) == 0u) return;   // the whole group, so the whole workgroup
  const uint32_t excl = incl - val;
  const uint32_t base_full = a.group_counts[g], base_tomb = a.group_counts[(size_t)a.groups + g];
  const uint32_t base_raw = a.offsets ? a.group_counts[2 * (size_t)a.groups + g] : 0u;
  unsigned long long w_full[kSubmapPer], w_tomb[kSubmapPer];
  uint32_t b_full[kSubmapPer], b_tomb[kSubmapPer], b_raw[kSubmapPer];
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k) {   // every lane takes part in the cross-lane reads
    const int q = (int)(k * (kSubmapBlock / 64u) + wave);
    w_full[k] = __shfl(mine, q, 64);
    w_tomb[k] = __shfl(mine, 16 + q, 64);
    b_full[k] = __shfl(excl, q, 64);
    b_tomb[k] = __shfl(excl, 16 + q, 64);
    b_raw[k] = __shfl(excl, 32 + q, 64);
  }
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k) {
    if ((w_full[k] | w_tomb[k]) == 0ull) continue;   // the wave's 64 slots of this turn: nothing here (the same for every lane)
    const uint64_t wave_slot = (uint64_t)g * kSubmapGroupSlots + kSubmapBlock * k + 64u * wave;
    const uint32_t slot = (uint32_t)(wave_slot + lane);
    const bool full = (w_full[k] >> lane) & 1ull;
    if ((w_tomb[k] >> lane) & 1ull) {
      const uint32_t rank = base_tomb + b_tomb[k] + (uint32_t)__popcll(w_tomb[k] & below);
      if (rank < a.tomb_capacity) a.tomb_slots[rank] = slot;
    }
    const uint32_t first = base_full + b_full[k];
    if (full) {
      const uint32_t rank = first + (uint32_t)__popcll(w_full[k] & below);
      if (rank < a.full_capacity) a.full_slots[rank] = slot;
    }
    if (w_full[k] == 0ull) continue;
    if (a.offsets) {   // the same for every lane: the prefix sum of the counts in slot order
      const uint32_t c = full ? (uint32_t)a.table[slot].count : 0u;
      uint32_t upto = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(upto, d, 64);
        if (lane >= (uint32_t)d) upto += up;
      }
      if (full) a.offsets[slot] = base_raw + b_raw[k] + upto - c;
    }
    const uint32_t part = lane & 7u;
#pragma unroll 1
    for (uint32_t pass = 0; pass < 8u; ++pass) {
      const uint32_t r = pass * 8u + (lane >> 3);   // which of the wave's 64 slots
      if (!((w_full[k] >> r) & 1ull)) continue;
      const uint32_t rank = first + (uint32_t)__popcll(w_full[k] & ((1ull << r) - 1ull));
      if (rank >= a.full_capacity) continue;   // the host sizes the outputs for every voxel it knows of; this is the belt
      uint4 v = reinterpret_cast<const uint4*>(a.table + wave_slot + r)[part];
      if (part == 7u) v.z = v.w = 0u;          // {count, spare}: the spare word is the launches' scratch, zero in a blob
      reinterpret_cast<uint4*>(a.records + rank)[part] = v;
    }
  }
}

// The live entries of the log to their places in the raw section (raw_scatter_kernel without the keys).
__global__ void checkpoint_raw_kernel(const RawPoint* __restrict__ log, uint32_t upper, const uint32_t* ctr,
                                      const VoxelRecord* __restrict__ table, uint64_t slots,
                                      const uint32_t* __restrict__ offsets, uint32_t capacity, double* __restrict__ points) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t used = ctr[0] < upper ? ctr[0] : upper;
  if (e >= used) return;
  const RawPoint p = log[e];
  if ((uint64_t)p.slot >= slots) return;   // see raw_compact_kernel
  const VoxelRecord* rec = table + p.slot;
  if (rec->state != SLOT_FULL || p.ordinal >= rec->count) return;  // dead (evicted / erased voxel)
  const uint64_t pos = (uint64_t)offsets[p.slot] + p.ordinal;
  if (pos >= capacity) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) points[3 * pos + k] = p.xyz[k];
}

// ---- the restore ----
// SCATTER.  Eight lanes per record, 16 bytes each; behind them one lane per tombstone writes a head whose state is
// SLOT_TOMB (nothing reads a tombstone's other bytes).  Every slot passed the host's check; the compare is the belt.
__global__ void restore_scatter_kernel(RestoreArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t parts = 8ull * a.voxels;
  if (i < parts) {
    const uint64_t j = i >> 3;
    const uint32_t part = (uint32_t)i & 7u, slot = a.full_slots[j];
    if ((uint64_t)slot >= a.slots) return;
    reinterpret_cast<uint4*>(a.table + slot)[part] = reinterpret_cast<const uint4*>(a.records + j)[part];
    return;
  }
  const uint64_t t = i - parts;
  if (t >= a.tombstones) return;
  const uint32_t slot = a.tomb_slots[t];
  if ((uint64_t)slot >= a.slots) return;
  *reinterpret_cast<int4*>(a.table + slot) = make_int4(0, 0, 0, SLOT_TOMB);
}
// a record's count as the log's rebuild takes it: never beyond the points the blob holds (rule 14 says their sum is that)
__device__ __forceinline__ uint32_t restore_count(const RestoreArgs& a, uint64_t j) {
  if (j >= a.voxels) return 0u;
  const uint64_t c = a.records[j].count;
  return c < a.raw_points ? (uint32_t)c : a.raw_points;
}
// the sum over a workgroup of kRestoreBlock lanes of v (to every lane), and what lies before this lane's
__device__ __forceinline__ uint32_t restore_block_scan(uint32_t v, uint32_t* wave_sum, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += up;
  }
  if (lane == 63u) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t before = 0u, all = 0u;
  for (uint32_t w = 0; w < kRestoreBlock / 64u; ++w) {
    if (w < wave) before += wave_sum[w];
    all += wave_sum[w];
  }
  *total = all;
  return before + incl - v;
}
__global__ __launch_bounds__(kRestoreBlock) void restore_raw_count_kernel(RestoreArgs a) {
  __shared__ uint32_t wave_sum[kRestoreBlock / 64u];
  uint32_t total;
  (void)restore_block_scan(restore_count(a, (uint64_t)blockIdx.x * kRestoreBlock + threadIdx.x), wave_sum, &total);
  if (threadIdx.x == 0u) a.block_sums[blockIdx.x] = total;
}
// block_sums are exclusive offsets by now: record j's points go to offset[j] .. offset[j] + count
__global__ __launch_bounds__(kRestoreBlock) void restore_raw_fill_kernel(RestoreArgs a) {
  __shared__ uint32_t wave_sum[kRestoreBlock / 64u];
  const uint64_t j = (uint64_t)blockIdx.x * kRestoreBlock + threadIdx.x;
  const uint32_t c = restore_count(a, j);
  uint32_t total;
  const uint32_t at = a.block_sums[blockIdx.x] + restore_block_scan(c, wave_sum, &total);
  if (blockIdx.x == 0u && threadIdx.x == 0u) a.ctr[0] = a.raw_points;
  if (c == 0u) return;
  const uint32_t slot = a.full_slots[j];
  for (uint32_t o = 0; o < c; ++o) {
    const uint64_t pos = (uint64_t)at + o;
    if (pos >= a.raw_points || pos >= a.log_capacity) return;
    RawPoint p;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.xyz[k] = a.raw[3 * pos + k];
    p.slot = slot;
    p.ordinal = o;
    a.log[pos] = p;
  }
}

// ---- map merge (include/vgicp_hip_map_merge.h states the rule operation by operation; this restates it).  MARK and SCAN
// are the submap's above, launched as they are ----
// MOVE-AND-CLAIM.  The ranks as in the submap's EMIT, taken densely (below); the record moved by the same two device
// functions; the key of the moved mean at the destination's voxel size; the insertion's claim loop; one 128-byte line per
// contributor at its rank.
// Before that every workgroup helps to fill the sort's input behind the last rank: SCAN's total is on the device only.
__global__ __launch_bounds__(kSubmapBlock) void merge_move_kernel(MergeArgs m) {
  static_assert(kSubmapGroupWords <= 64u, "a wave holds its group's ballots, one per lane");
  static_assert(kSubmapGroupSlots <= 65536u, "a slot's place in its group fits 16 bits");
  __shared__ uint32_t sums[2];
  __shared__ uint16_t list[kSubmapGroupSlots];
  const SubmapArgs& a = m.sub;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid < 2u) sums[tid] = 0u;
  const unsigned long long total = a.totals[0];
  const uint64_t selected = total < (unsigned long long)m.n ? total : m.n;
  for (uint64_t t = selected + (uint64_t)blockIdx.x * kSubmapBlock + tid; t < m.n; t += (uint64_t)gridDim.x * kSubmapBlock) {
    m.slot_in[t] = kNoSlot;
    m.idx_in[t] = (uint32_t)t;
  }
  const unsigned long long mine = lane < kSubmapGroupWords ? a.ballots[(size_t)blockIdx.x * kSubmapGroupWords + lane] : 0ull;
  const uint32_t pc = (uint32_t)__popcll(mine);
  uint32_t incl = pc;
#pragma unroll
  for (int d = 1; d < (int)kSubmapGroupWords; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += up;
  }
  if (__shfl(incl, (int)kSubmapGroupWords - 1, 64) == 0u) return;   // the whole group, so the whole workgroup
  const uint32_t excl = incl - pc;
  const uint32_t base = a.group_counts[blockIdx.x];
  unsigned long long word[kSubmapPer];
  uint32_t before[kSubmapPer];
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k) {   // every lane takes part in the cross-lane reads
    const int q = (int)(k * (kSubmapBlock / 64u) + wave);
    word[k] = __shfl(mine, q, 64);
    before[k] = __shfl(excl, q, 64);
  }
  // The group's selected slots, in rank order, into LDS; then the lanes take them DENSELY, one contributor per lane: the
  // claim is a chain of dependent memory round trips per wave, and a table is mostly empty slots — taken where the bits
  // stand (a wave per 64 slots and turn) a wave would run that chain for one or a few lanes at a time
#pragma unroll
  for (uint32_t k = 0; k < kSubmapPer; ++k)
    if ((word[k] >> lane) & 1ull)
      list[before[k] + (uint32_t)__popcll(word[k] & ((1ull << lane) - 1ull))] = (uint16_t)(kSubmapBlock * k + tid);
  const uint32_t group_total = __shfl(incl, (int)kSubmapGroupWords - 1, 64);   // <= kSubmapGroupSlots
  __syncthreads();   // behind the list, and behind the zeroing of sums
  uint32_t created = 0, lost = 0;
#pragma unroll 1
  for (uint32_t at = tid; at < group_total; at += kSubmapBlock) {
    const size_t rank = (size_t)base + at;
    if (rank >= m.n) continue;   // the host sizes the scratch for every voxel of the source; this is the belt
    const VoxelRecord* rec = a.table + ((uint64_t)blockIdx.x * kSubmapGroupSlots + list[at]);
    const double2* pay = reinterpret_cast<const double2*>(rec->mean);   // 16-byte aligned
    const double2 p0 = pay[0], p1 = pay[1], p2 = pay[2], p3 = pay[3], p4 = pay[4], p5 = pay[5];
    const unsigned long long count = rec->count;
    const double C[9] = {p1.y, p2.x, p2.y, p3.x, p3.y, p4.x, p4.y, p5.x, p5.y};
    double v[kScanPlanes];
    transform_point(a.pose, a.pose + 9, p0.x, p0.y, p1.x, v);
    rotate_cov_exact(a.pose, C, v + 3);
    bool fresh = false;
    const uint32_t found = claim_slot(m.table, m.mask, voxel_coord(v[0], m.voxel_size), voxel_coord(v[1], m.voxel_size),
                                      voxel_coord(v[2], m.voxel_size), fresh);
    created += fresh ? 1u : 0u;
    lost += found == kNoSlot ? 1u : 0u;
    double2* out = reinterpret_cast<double2*>(m.moved + rank);   // the line: 6 x 16 bytes of statistics, then {count, slot}
#pragma unroll
    for (int e = 0; e < 6; ++e) out[e] = make_double2(v[2 * e], v[2 * e + 1]);
    m.moved[rank].count = count;
    m.moved[rank].slot = found;
    m.slot_in[rank] = found;
    m.idx_in[rank] = (uint32_t)rank;
  }
  // one atomic per workgroup and counter
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    created += __shfl_down(created, d, 64);
    lost += __shfl_down(lost, d, 64);
  }
  if (lane == 0u) {
    if (created) atomicAdd(&sums[0], created);
    if (lost) atomicAdd(&sums[1], lost);
  }
  __syncthreads();
  if (tid < 2u && sums[tid]) atomicAdd(&m.counters[tid], sums[tid]);
}

// one entry of the fold: (nn * x + cc * y) / n1, every operation rounded once
__device__ __forceinline__ double merge_entry(double nn, double x, double cc, double y, double n1) {
#pragma clang fp contract(off)
  const double a = nn * x, b = cc * y;
  const double s = a + b;
  return s / n1;
}
// The workgroup's 64-bit sums of every lane's two values, for thread 0 (every thread of a kBlock workgroup calls this).
__device__ __forceinline__ void merge_block_sums(unsigned long long& u, unsigned long long& v) {
  __shared__ unsigned long long part[2][kBlock / 64];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    u += __shfl_down(u, (unsigned int)d, 64);
    v += __shfl_down(v, (unsigned int)d, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
    part[0][threadIdx.x >> 6] = u;
    part[1][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  u = v = 0ull;
#pragma unroll
  for (uint32_t w = 0; w < kBlock / 64; ++w) {
    u += part[0][w];
    v += part[1][w];
  }
}
// APPLY.  The head of the segment that starts at sorted position j folds its contributors, in rank order, into the
// destination record's state in registers and writes the record once — not at all when nothing was accepted.  Every slot
// and every rank read from the sort's output is checked against its capacity before it indexes anything.
__global__ __launch_bounds__(kBlock) void merge_apply_kernel(MergeArgs m) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t slot = kNoSlot;
  bool head = false;
  if (j < m.n) {
    slot = m.slot_out[j];
    head = slot != kNoSlot && slot <= m.mask && !(j > 0 && m.slot_out[j - 1] == slot);
  }
  bool updated = false;
  unsigned long long frozen = 0ull, points = 0ull;
  if (head) {
    VoxelRecord* rec = m.table + slot;
    const uint64_t before = rec->count;
    uint64_t count = before;
    double s[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = rec->mean[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[3 + k] = rec->cov[k];
    bool accepted = false;
    for (uint32_t q = j; q < m.n && m.slot_out[q] == slot; ++q) {
      const uint32_t i = m.idx_out[q];
      if (i >= m.n) continue;
      if (m.max_count != 0ull && count >= m.max_count) {   // frozen: the contributor's line is not read
        ++frozen;
        continue;
      }
      const double2* in = reinterpret_cast<const double2*>(m.moved + i);
      double c[12];
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        const double2 p = in[e];
        c[2 * e] = p.x;
        c[2 * e + 1] = p.y;
      }
      const uint64_t cnt = m.moved[i].count;
      if (count == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] = c[k];
        count = cnt;
      } else {
        const double nn = (double)count, cc = (double)cnt, n1 = (double)(count + cnt);
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] = merge_entry(nn, s[k], cc, c[k], n1);
        count += cnt;
      }
      points += cnt;
      accepted = true;
    }
    if (accepted) {
#pragma unroll
      for (int k = 0; k < 3; ++k) rec->mean[k] = s[k];
#pragma unroll
      for (int k = 0; k < 9; ++k) rec->cov[k] = s[3 + k];
      rec->count = count;
      updated = before != 0;
    }
  }
  // one atomic per workgroup and counter
  const int n_updated = __syncthreads_count(updated ? 1 : 0);
  merge_block_sums(frozen, points);
  if (threadIdx.x == 0u) {
    if (n_updated) atomicAdd(&m.totals[4], (unsigned long long)n_updated);
    if (frozen) atomicAdd(&m.totals[5], frozen);
    if (points) atomicAdd(&m.totals[6], points);
  }
}

}  // namespace

size_t map_insert_scratch_bytes(uint32_t n) {
  const uint32_t m = n ? n : 1;
  return align256((size_t)m * 3 * sizeof(double)) + align256((size_t)m * 9 * sizeof(double)) +
         4 * align256((size_t)m * sizeof(uint32_t)) + align256(sortk::split_bytes(m, sizeof(uint32_t))) + 256;
}

hipError_t launch_map_insert(hipStream_t s, VoxelRecord* table, uint32_t mask, double voxel_size,
                             const double* points_aos, const double* covs_aos, uint32_t n,
                             const double pose12[12], uint64_t max_points, void* scratch,
                             size_t scratch_bytes, uint32_t* counters, bool short_lists, const RawLog& raw,
                             const uint8_t* keep) {
  if (n == 0) return hipSuccess;
  if (scratch_bytes < map_insert_scratch_bytes(n)) return hipErrorInvalidValue;
  InsertScratch w = carve(scratch, n);
  Pose12 pose;
  for (int k = 0; k < 12; ++k) pose.v[k] = pose12[k];
  if (short_lists) {
    counted_launch(insert_prepare_kernel<true>, dim3(blocks_for(n, 256)), dim3(256), 0, s, table, mask, voxel_size, points_aos,
                   covs_aos, n, pose, w.wpts, w.wcovs, w.slot_in, w.idx_in, counters, keep);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (raw.entries) {
      counted_launch(insert_apply_list_kernel<true>, dim3(blocks_for(n, 256)), dim3(256), 0, s, table, w.slot_in, w.idx_in, n,
                     w.wpts, w.wcovs, max_points, raw);
    } else {
      counted_launch(insert_apply_list_kernel<false>, dim3(blocks_for(n, 256)), dim3(256), 0, s, table, w.slot_in, w.idx_in, n,
                     w.wpts, w.wcovs, max_points, raw);
    }
    return hipGetLastError();
  }
  counted_launch(insert_prepare_kernel<false>, dim3(blocks_for(n, 256)), dim3(256), 0, s, table, mask, voxel_size, points_aos,
                 covs_aos, n, pose, w.wpts, w.wcovs, w.slot_in, w.idx_in, counters, keep);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // stable: equal slots keep ascending point index = scan order (the inputs are scratch from here on)
  e = sortk::sort_pairs(w.slot_in, w.idx_in, w.slot_out, w.idx_out, w.split, n, s);
  if (e != hipSuccess) return e;
  g_kernel_launches += sortk::launches_for(n);
  if (raw.entries) {
    counted_launch(insert_apply_kernel<true>, dim3(blocks_for(n, 256)), dim3(256), 0, s, table, w.slot_out, w.idx_out, n, w.wpts,
                   w.wcovs, max_points, raw);
  } else {
    counted_launch(insert_apply_kernel<false>, dim3(blocks_for(n, 256)), dim3(256), 0, s, table, w.slot_out, w.idx_out, n, w.wpts,
                   w.wcovs, max_points, raw);
  }
  return hipGetLastError();
}

hipError_t launch_map_evict(hipStream_t s, VoxelRecord* table, uint64_t slots, double voxel_size,
                            const double position[3], double distance, uint32_t* counters) {
  counted_launch(evict_kernel, dim3(blocks_for(slots, 256)), dim3(256), 0, s, table, slots, voxel_size, position[0], position[1],
                 position[2], distance, counters);
  return hipGetLastError();
}

hipError_t launch_map_carve(hipStream_t s, const CarveArgs& args) {
  if (!args.removed || args.slots == 0 || (args.slots & (args.slots - 1)) != 0) return hipErrorInvalidValue;
  if (args.n == 0) return hipSuccess;   // no point: no mark, and nothing for the sweep to find
  counted_launch(carve_mark_kernel, dim3(blocks_for(args.n, kBlock)), dim3(kBlock), 0, s, args);
  counted_launch(carve_sweep_kernel, dim3(blocks_for(args.slots, kBlock)), dim3(kBlock), 0, s, args);
  return hipGetLastError();
}

hipError_t launch_map_rays(hipStream_t s, const RayArgs& args) {
  if (!args.table || !args.bits || !args.counts || !args.poses || args.slots < 32 || (args.slots & (args.slots - 1)) != 0)
    return hipErrorInvalidValue;
  if (args.n_poses == 0 || args.n_poses > 65535u || args.stride == 0) return hipErrorInvalidValue;
  if (args.n_poses != 1 && (args.status || args.range || args.hit_key || args.steps)) return hipErrorInvalidValue;
  if (args.n == 0) return hipSuccess;
  const dim3 grid(blocks_for(args.n, kBlock), args.n_poses);
  counted_launch(rays_confirm_kernel, grid, dim3(kBlock), 0, s, args);
  counted_launch(rays_walk_kernel, grid, dim3(kBlock), 0, s, args);
  return hipGetLastError();
}

hipError_t launch_map_export(hipStream_t s, const VoxelRecord* table, uint64_t slots, uint32_t capacity,
                             int32_t* keys, double* means, double* covs, uint64_t* counts,
                             uint32_t* counters) {
  counted_launch(export_kernel, dim3(blocks_for(slots, 256)), dim3(256), 0, s, table, slots, capacity, keys, means, covs, counts,
                 counters);
  return hipGetLastError();
}

hipError_t launch_submap(hipStream_t s, const SubmapArgs& a, unsigned long long* totals_host) {
  counted_launch(submap_mark_kernel, dim3(a.groups), dim3(kSubmapBlock), 0, s, a);
  counted_launch(submap_scan_kernel, dim3(1), dim3(1024), 0, s, a.group_counts, a.groups, a.totals, totals_host);
  counted_launch(submap_emit_kernel, dim3(a.groups), dim3(kSubmapBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_map_merge(hipStream_t s, const MergeArgs& m, unsigned long long* totals_host) {
  const SubmapArgs& a = m.sub;
  if (!m.table || !a.table || m.n == 0 || a.groups == 0 || ((uint64_t)m.mask & ((uint64_t)m.mask + 1)) != 0) return hipErrorInvalidValue;
  // the plan sizes the splitters' room without the sort's header: it must hold what the sort asks for
  if (merge_sort_split_bytes(m.n) < sortk::split_bytes(m.n, sizeof(uint32_t))) return hipErrorInvalidValue;
  counted_launch(submap_mark_kernel, dim3(a.groups), dim3(kSubmapBlock), 0, s, a);
  counted_launch(submap_scan_kernel, dim3(1), dim3(1024), 0, s, a.group_counts, a.groups, a.totals, totals_host);
  counted_launch(merge_move_kernel, dim3(a.groups), dim3(kSubmapBlock), 0, s, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // stable: equal slots keep ascending rank = the source's slot order (the inputs are scratch from here on)
  e = sortk::sort_pairs(m.slot_in, m.idx_in, m.slot_out, m.idx_out, m.split, m.n, s);
  if (e != hipSuccess) return e;
  g_kernel_launches += sortk::launches_for(m.n);
  counted_launch(merge_apply_kernel, dim3(blocks_for(m.n, kBlock)), dim3(kBlock), 0, s, m);
  return hipGetLastError();
}

hipError_t launch_checkpoint(hipStream_t s, const CheckpointArgs& a, unsigned long long* totals_host) {
  if (!a.table || a.groups == 0 || a.slots != (uint64_t)a.groups * kSubmapGroupSlots) return hipErrorInvalidValue;
  counted_launch(checkpoint_mark_kernel, dim3(a.groups), dim3(kSubmapBlock), 0, s, a);
  counted_launch(checkpoint_scan_kernel, dim3(1), dim3(1024), 0, s, a.group_counts, a.groups, a.word_raw ? 3u : 2u, a.totals, totals_host);
  counted_launch(checkpoint_emit_kernel, dim3(a.groups), dim3(kSubmapBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_checkpoint_raw(hipStream_t s, const RawPoint* log, uint32_t upper, const uint32_t* ctr, const VoxelRecord* table,
                                 uint64_t slots, const uint32_t* offsets, uint32_t capacity, double* points) {
  if (upper == 0) return hipSuccess;
  counted_launch(checkpoint_raw_kernel, dim3(blocks_for(upper, 256)), dim3(256), 0, s, log, upper, ctr, table, slots, offsets,
                 capacity, points);
  return hipGetLastError();
}

hipError_t launch_restore(hipStream_t s, const RestoreArgs& a) {
  const uint64_t lanes = 8ull * a.voxels + a.tombstones;
  if (lanes > 0) counted_launch(restore_scatter_kernel, dim3(blocks_for(lanes, 256)), dim3(256), 0, s, a);
  if (a.log && a.voxels > 0) {
    const uint32_t blocks = restore_blocks(a.voxels);
    counted_launch(restore_raw_count_kernel, dim3(blocks), dim3(kRestoreBlock), 0, s, a);
    counted_launch(checkpoint_scan_kernel, dim3(1), dim3(1024), 0, s, a.block_sums, blocks, 1u, a.totals, (unsigned long long*)nullptr);
    counted_launch(restore_raw_fill_kernel, dim3(blocks), dim3(kRestoreBlock), 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_raw_compact(hipStream_t s, const RawPoint* src, uint32_t src_upper, const uint32_t* ctr,
                              const VoxelRecord* table, uint64_t slots, const uint32_t* claimed, RawPoint* dst,
                              uint32_t dst_capacity, uint32_t* dst_ctr) {
  if (src_upper == 0) return hipSuccess;
  counted_launch(raw_compact_kernel, dim3(blocks_for(src_upper, 256)), dim3(256), 0, s, src, src_upper, ctr, table, slots,
                 claimed, dst, dst_capacity, dst_ctr);
  return hipGetLastError();
}

hipError_t launch_raw_offsets(hipStream_t s, const VoxelRecord* table, uint64_t slots, uint32_t* offsets, uint32_t* total) {
  counted_launch(raw_offsets_kernel, dim3(blocks_for(slots, 256)), dim3(256), 0, s, table, slots, offsets, total);
  return hipGetLastError();
}

hipError_t launch_raw_scatter(hipStream_t s, const RawPoint* log, uint32_t upper, const uint32_t* ctr,
                              const VoxelRecord* table, uint64_t slots, const uint32_t* offsets, uint32_t capacity,
                              int32_t* keys, double* points) {
  if (upper == 0) return hipSuccess;
  counted_launch(raw_scatter_kernel, dim3(blocks_for(upper, 256)), dim3(256), 0, s, log, upper, ctr, table, slots, offsets,
                 capacity, keys, points);
  return hipGetLastError();
}

}  // namespace vgicp
