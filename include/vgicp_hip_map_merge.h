/* vgicp_hip_map_merge.h — extension of the C ABI (vgicp_hip.h): MAP MERGE.  The voxels of a region of one device map
 * folded into another device map, each weighted by the points it stands for, on the device.
 *
 * vgicp_scan_from_map of vgicp_hip_map_submap.h answers "where is this piece of map in that map?"; once that pose is
 * known — a loop closure, a second session registered against a first, a map re-anchored after a correction — the two
 * maps are to become one.  vgicp_scan_from_map + vgicp_map_insert_resident inserts every source voxel as ONE point: a
 * voxel that stands for 40 returns moves the destination's running mean as much as one that stands for a single return.
 * vgicp_map_export delivers the counts to the host, but nothing takes them back.  This call goes from table to table.
 *
 * THE RULE, operation by operation (the kernels in vgicp_mapupdate.hip and tests/map_merge_reference.py restate it; IEEE
 * double arithmetic with NO fused multiply-add, every product, sum and quotient rounded once).
 *
 *   SELECTION.  vgicp_scan_from_map's at level 0: a FULL record of src with key K and count c is a CONTRIBUTOR iff
 *       vgicp_map_evict at `center` with distance_threshold = radius would keep it and (min_count <= 1 || c >= min_count).
 *       The device function that decides it is the one eviction runs; voxels, selected, too_far and too_few are the four
 *       counts of vgicp_submap_stats for the same parameters (selected is its `points`).
 *   TRANSFORM.  vgicp_scan_from_map's, by the same device functions: frame = (R, t),
 *         m' = ((R[.,0] m0 + R[.,1] m1) + R[.,2] m2) + t       C' = (R C) R^T, every entry left to right
 *       Contributor j, moved, is bit for bit scan point j of vgicp_scan_from_map with the same center, radius, min_count
 *       and frame; its count c is the record's.
 *   KEY.  The destination voxel of a contributor is the map's own key of its MOVED MEAN at dst's voxel size, per axis
 *       k_a = (int32) floor(m'_a / voxel_size), as the insertion keys a point.
 *   ORDER.  The contributors of one destination voxel are taken in ascending slot index of the source table.
 *   FOLD.  The state (count, mean, cov) of a destination voxel starts as its record when the voxel exists and at count 0
 *       otherwise.  For each contributor (c, m', C') in order:
 *         if (max_count != 0 && count >= max_count)   not accepted: `frozen` counts it, the state stays;
 *         else if (count == 0)                        mean = m', cov = C' bit for bit, count = c;
 *         else   nn = (double)count, cc = (double)c, n1 = (double)(count + c);
 *                every one of the twelve entries x becomes (nn * x + cc * x') / n1;   count += c.
 *       With c == 1 the product cc * x' is exact, so a contributor of one point is Voxel::addPoint bit for bit: a source
 *       whose voxels all hold one point merges to exactly what vgicp_map_insert_resident of its vgicp_scan_from_map scan
 *       leaves at max_points_per_voxel = max_count.  A destination voxel that is frozen from the start is not written at
 *       all.  A fresh voxel always accepts its first contributor (0 >= max_count never holds for a cap), so no record is
 *       left at count 0.  The cap stops a voxel from accepting further contributors; it does not split one: the count
 *       may pass max_count by the last accepted contributor's points.
 *   Tombstones of dst are passed over and never claimed, as in the insertion.  The spare word of every record is left as
 *   an insertion leaves it.
 *
 * WHAT THE CALL DOES TO THE CONTEXTS.  dst's map changes as by an insertion: the map version advances (the levels and
 * the dense copy rebuild lazily), the voxel count grows by `created`; the table grows first, by the insertion's rule, for
 * as many new voxels as src holds.  dst's resident scan, its scan generation and its fetch state are not touched.  src is
 * only read: its table, its scan and its scan generation stay.  What is pending in either context is settled first.
 * There is ONE host synchronisation, at the end, which brings the counts (a table that has to grow synchronises as it
 * does for an insertion).
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The entry point lives in a library of its own beside the module, libvgicp_hip_map_merge.so,
 * which links against libvgicp_hip.so and must come from the same build.  VGICP_ABI_VERSION is unchanged, and no
 * vgicp_set_option number is introduced.  Nothing of this header is allocated before the first call.  Single device; no
 * asynchronous form; the source is the map itself, not one of its levels; a destination that keeps raw points is
 * refused. */
#ifndef VGICP_HIP_MAP_MERGE_H_
#define VGICP_HIP_MAP_MERGE_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vgicp_merge_params {   /* 184 bytes, LP64 */
  double   center[3];   /* in the SOURCE map's frame */
  double   radius;      /* >= 0, or +infinity: the whole map */
  double   frame[16];   /* rigid transform source map -> destination map, column-major */
  uint64_t min_count;   /* source voxels with fewer points are left out; 0 and 1 take all */
  uint64_t max_count;   /* a destination voxel holding >= max_count points accepts nothing more; 0: no cap */
  uint64_t reserved;    /* 0 */
} vgicp_merge_params;

typedef struct vgicp_merge_stats {    /* 88 bytes, LP64 */
  uint64_t voxels, selected, too_far, too_few;   /* as vgicp_submap_stats names them (selected = its `points`) */
  uint64_t created;     /* destination voxels that did not exist before the call */
  uint64_t updated;     /* destination voxels that existed and accepted at least one contributor */
  uint64_t frozen;      /* selected source voxels that a capped destination voxel did not accept */
  uint64_t points;      /* sum of the accepted contributors' counts */
  int32_t  launches, reserved;   /* kernel launches of this call; 0 */
  double   seconds, device_seconds;   /* host wall time of the call; event span around its launches */
} vgicp_merge_stats;

/* The selected voxels of src's map, moved by params->frame, are folded into dst's map.  stats is optional.
 *
 * REFUSALS, in this order; VGICP_ERR_BAD_ARGUMENT unless stated.  A refused call changes nothing in either context:
 *   1. NULL dst, src or params;
 *   2. dst or src was not made by this build of the module;
 *   3. dst or src is a multi-device context (vgicp_create_multi), has a communicator or is peer-connected;
 *   4. dst == src;
 *   5. dst and src are on different devices;
 *   6. reserved != 0;
 *   7. an entry of center or frame that is not finite;
 *   8. radius NaN, negative or -infinity;
 *   9. dst or src has no map (VGICP_ERR_NOT_READY);
 *  10. the voxel sizes of dst and src differ in any bit;
 *  11. dst keeps raw points (VGICP_OPTION_MAP_RAW_POINTS): a merged voxel has no point list to keep;
 *  12. once what is pending in both contexts has been settled: the source holds more voxels than a resident scan may
 *      hold (the limit of vgicp_scan_from_map);
 *  13. once what is pending in both contexts has been settled: the table dst would have to grow to passes 2^32 slots.
 * An empty source returns VGICP_OK with every count zero and without a launch.
 *
 * LAUNCHES, all on dst's stream behind an event of src's, no host round trip between them.  MARK and SCAN over the source
 * table are vgicp_scan_from_map's.  MOVE-AND-CLAIM: the ranks come from the ballots; a workgroup lists its selected slots
 * in rank order and its lanes take them densely, one contributor each: a lane transforms its
 * record, finds or claims the destination slot (the insertion's bounded claim loop) and writes the moved record, its
 * count and the slot at its rank into scratch, one 128-byte line per contributor.  SORT: the library's stable sort of
 * (slot, rank) by slot: the contributors of a voxel become one segment, in rank order = source slot order.  APPLY: the
 * head of a segment folds it in registers and writes the record once.  No workgroup waits for another but inside the
 * claim loop, which is bounded; every index read from device memory is checked against its capacity before it is used. */
int vgicp_map_merge(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_merge_params* params,
                    vgicp_merge_stats* stats /* optional */);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_MERGE_H_ */
