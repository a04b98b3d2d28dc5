/* vgicp_hip_map_carve.h — extension of the C ABI (vgicp_hip.h): FREE-SPACE CARVING.  Remove from the map the voxels that
 * the resident scan sees through.
 *
 * The map can grow (vgicp_map_insert_*), forget by distance (vgicp_map_evict) and keep bad points out
 * (vgicp_hip_map_gated.h).  What it holds already stays until the sensor has moved away: a parked car that drove off, a
 * pedestrian averaged into a dozen voxels.  Every sweep says where they are not: a return at range r says that the ray
 * was free from 0 to r, and a FULL voxel inside that free space contradicts what the sensor has just measured.  The
 * calls below cast the resident scan's rays through the voxel table at a pose and turn the voxels that enough rays
 * crossed into tombstones — on the device, in the stream, without the scan ever visiting the host.
 *
 * THE RULE, operation by operation (the kernels in vgicp_mapupdate.hip and tests/map_carve_reference.py restate it; all
 * of it is IEEE double arithmetic with NO fused multiply-add, every product, sum, quotient and square root rounded once).
 * Inputs: the resident scan of n points p_i in its own frame, the pose `transform` T = (R, t), the map's voxel size h,
 * and vgicp_carve_params.  The deskewed sweep is treated as cast from ONE origin: the approximation the prepared scan
 * itself makes.
 *
 *   x |-> T x   is the insertion's transform:  ((R[.,0] x0 + R[.,1] x1) + R[.,2] x2) + t   per row
 *   key(x)      is the insertion's key:        floor(x / h) per axis; DEFINED iff all three are within +-2^30
 *
 * SHIELD.  For every point i (all of them, whatever `stride`): e_i = T p_i.  If key(e_i) is defined and the voxel with
 * that key is FULL, it is SHIELDED: a voxel that holds a return of this scan is never carved by this scan.  (This is
 * what keeps the ground plane under grazing rays.)
 *
 * RAY.  Only points with i % stride == 0 cast a ray.
 *   o = T origin,   d = e_i - o,   len = sqrt((dx dx + dy dy) + dz dz),   t_stop = min(len - margin, max_range) / len
 *   There is no ray unless t_stop > 0, every entry of d is finite and key(o) is defined.
 *   The ray visits the voxel k = key(o) first.  Then, per axis a:
 *       tMax_a = d_a == 0 ? +infinity : ((double)(k_a + (d_a > 0 ? 1 : 0)) * h - o_a) / d_a
 *   and, at most  3 * ceil((t_stop * len) / h) + 3  times:
 *       a = the axis with the smallest tMax; ties go to x before y before z
 *       stop unless tMax_a < t_stop
 *       k_a += (d_a > 0 ? 1 : -1);  visit k;  tMax_a is formed anew from the new k_a by the expression above
 *   (the classic voxel traversal of Amanatides and Woo, with the boundary recomputed from the integer key at every step
 *   instead of accumulated).  A voxel is thus visited iff the parameter at which the ray enters it is < t_stop; the
 *   walk visits a voxel at most once per ray.  Every visited voxel that is FULL gets ONE HIT from this ray, so a
 *   voxel's hits are a count of distinct rays and do not depend on the order in which the device runs them.
 *
 * REMOVAL.  A FULL voxel with hits >= min_hits that is not shielded becomes a tombstone, exactly as vgicp_map_evict makes
 * one: its raw points (vgicp_hip_map_points.h) die with it, the dense copy goes out of date, vgicp_map_size shrinks.
 * Nothing else in the table changes: the survivors' records are bit for bit what they were.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The three entry points live in a library of their own beside the module,
 * libvgicp_hip_map_carve.so, which links against libvgicp_hip.so and must come from the same build (a context of
 * another build is refused).  VGICP_ABI_VERSION is unchanged, and no vgicp_set_option number is introduced. */
#ifndef VGICP_HIP_MAP_CARVE_H_
#define VGICP_HIP_MAP_CARVE_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VGICP_CARVE_MAX_STEPS 4096   /* max_range / voxel_size may not exceed this: the bound of a ray's walk */

typedef struct vgicp_carve_params {   /* 48 bytes, LP64 */
  double   origin[3];   /* the sensor's origin in the scan's frame: the extrinsic translation the preparation applied;
                           zero for a scan in the sensor frame */
  double   margin;      /* metres a ray stops short of its return: finite, >= 0 */
  double   max_range;   /* metres a ray is followed at most: finite, > 0, at most VGICP_CARVE_MAX_STEPS voxel sizes */
  uint32_t min_hits;    /* rays that must cross a voxel: >= 1 */
  uint32_t stride;      /* every stride-th point casts a ray: >= 1 */
} vgicp_carve_params;

typedef struct vgicp_carve_stats {   /* 64 bytes, LP64 */
  uint64_t rays;        /* rays cast */
  uint64_t visits;      /* voxels stepped through, over all rays (FULL or not) */
  uint64_t touched;     /* FULL voxels with >= 1 hit */
  uint64_t shielded;    /* ... of which shielded */
  uint64_t removed;
  int32_t  launches, reserved;
  double   seconds, device_seconds;   /* host wall time of the call; event span around its two launches */
} vgicp_carve_stats;

/* Carve the map with the resident scan at the pose `transform`.  removed_keys (optional, room for `capacity` voxels, 3
 * int32 each, order unspecified): the call writes min(capacity, removed) keys and nothing behind them; *removed
 * (optional) is always the full count; the call has carved either way and returns VGICP_OK.  stats is optional.
 *
 * REFUSALS, in this order; VGICP_ERR_BAD_ARGUMENT unless stated.  A refused call writes nothing: not to the map, not to
 * the scan (its generation counter does not move), not to removed_keys, *removed or *stats:
 *   1. NULL ctx;
 *   2. a context that was not made by this build of the module;
 *   3. no map, or no resident scan (VGICP_ERR_NOT_READY);
 *   4. NULL transform or params;
 *   5. a transform or origin entry that is not finite;
 *   6. margin NaN, negative or infinite;
 *   7. max_range not finite or <= 0, or max_range / voxel_size > VGICP_CARVE_MAX_STEPS;
 *   8. min_hits == 0 or stride == 0;
 *   9. a multi-device context (vgicp_create_multi), a communicator or a peer-connected context, with a text in
 *      vgicp_last_error.
 *
 * TWO LAUNCHES on the context's stream with no host round trip between them: the MARK launch (one lane per point: the
 * shield lookup, and the point's ray if it casts one) and the SWEEP launch (one lane per slot: decide, write the
 * tombstone, clear the marks).  Pending work is settled first; then one host synchronisation of the call's own. */
int vgicp_map_carve_resident(vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params* params,
                             size_t capacity, int32_t* removed_keys /* optional, 3 per voxel, order unspecified */,
                             size_t* removed /* optional */, vgicp_carve_stats* stats /* optional */);

/* The same two launches, enqueued: settles only what vgicp_map_insert_resident_async settles, waits for nothing else,
 * refuses by rules 1 to 9.  Its counts go to running totals on the device that the next synchronisation of the context
 * reads together with a deferred insertion's (vgicp_map_size and every other call that needs the map's size settle
 * first).  Followed by vgicp_map_insert_resident_async in the same frame, the pair adds no host synchronisation. */
int vgicp_map_carve_resident_async(vgicp_ctx* ctx, const double transform[16], const vgicp_carve_params* params);

/* Rays cast and voxels removed by the carving calls of this context since the last vgicp_map_reset; either may be NULL.
 * Settles pending work first.  Refuses by rules 1 and 2. */
int vgicp_map_carve_totals(vgicp_ctx* ctx, uint64_t* rays, uint64_t* removed);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_CARVE_H_ */
