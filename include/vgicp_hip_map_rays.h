/* vgicp_hip_map_rays.h — extension of the C ABI (vgicp_hip.h): THE RAY REPORT.  The first map voxel on every ray of the
 * resident scan, read-only.
 *
 * Every other call over the resident scan looks at the voxel a point falls into.  This one looks along the line of sight:
 * a return in front of the map's first surface is a point that APPEARED (a pedestrian in front of a wall: unmatched, so
 * the d^2 gate of vgicp_hip_map_gated.h lets it into the map); a FULL voxel well in front of the return is something the
 * sensor sees THROUGH (what vgicp_map_carve_resident would remove: the counts are a dry run of it); and of two poses that
 * tie on fitness and cost, the one that puts map surfaces between the sensor and its returns has the blocked rays.
 *
 * THE RULE, operation by operation (the kernels in vgicp_mapupdate.hip and tests/map_rays_reference.py restate it; all
 * of it is IEEE double arithmetic with NO fused multiply-add, every product, sum, quotient and square root rounded once).
 * Inputs: the resident scan of n points p_i in its own frame, a pose T = (R, t), the map's voxel size h, and
 * vgicp_ray_params.  x |-> T x, key(x), o, d, len, the per-axis boundary, the axis choice, the step and the re-formed
 * tMax are free-space carving's, word for word (include/vgicp_hip_map_carve.h): one definition of the step serves both.
 *
 *   x |-> T x   is the insertion's transform:  ((R[.,0] x0 + R[.,1] x1) + R[.,2] x2) + t   per row
 *   key(x)      is the insertion's key:        floor(x / h) per axis; DEFINED iff all three are within +-2^30
 *
 * CONFIRM.  For every point i (all of them, whatever `stride`): e_i = T p_i.  If key(e_i) is defined and the voxel with
 * that key is FULL, that voxel is CONFIRMED for this pose: it holds a return of this scan.
 *
 * RAY.  Only points with i % stride == 0 cast a ray.
 *   o = T origin,   d = e_i - o,   len = sqrt((dx dx + dy dy) + dz dz)
 *   t_end   = min(len + beyond, max_range) / len
 *   t_front = (len - margin) / len
 *   There is no ray unless len > 0, t_end > 0, every entry of d is finite and key(o) is defined.
 *   The ray visits the voxel k = key(o) first, with the entry parameter t_in = 0.  Then, per axis a:
 *       tMax_a = d_a == 0 ? +infinity : ((double)(k_a + (d_a > 0 ? 1 : 0)) * h - o_a) / d_a
 *   and, at most  3 * ceil((t_end * len) / h) + 3  times:
 *       a = the axis with the smallest tMax; ties go to x before y before z
 *       stop unless tMax_a < t_end
 *       t_in = tMax_a;  k_a += (d_a > 0 ? 1 : -1);  visit k;  tMax_a is formed anew from the new k_a by the expression above
 *   The walk STOPS at the first visited voxel that is FULL (tested at every visit, key(o) included).  That voxel is the
 *   HIT, with key k_hit and entry parameter t_in.
 *
 * CLASS.  One byte per point, decided in this order:
 *   0  VGICP_RAY_NO_RAY      the point cast no ray
 *   1  VGICP_RAY_OPEN        no FULL voxel was visited
 *   2  VGICP_RAY_OWN         key(e_i) is defined and k_hit == key(e_i)
 *   3  VGICP_RAY_BEHIND      t_in >= 1.0: the map's surface lies behind the return — the point appeared
 *   4  VGICP_RAY_CONFIRMED   the HIT is confirmed: another return of this scan lies in it (a grazing ray over ground)
 *   5  VGICP_RAY_BLOCKED     t_in < t_front: the map holds something the sensor sees through
 *   6  VGICP_RAY_NEAR        everything else: a HIT within `margin` in front of the return
 *
 * Per point (each plane optional, n entries): status; range = t_in * len as ONE product, the bit pattern
 * 0x7FF8000000000000 with no HIT; hit_key, INT32_MIN three times with no HIT; steps = the voxels visited, 0 with no ray.
 * Per pose: vgicp_ray_counts.
 *
 * READ-ONLY.  The table's bytes do not change, the scan's generation counter does not move, the map's version is not
 * bumped (the dense copy stays valid).  Confirmation therefore does not go into the records' spare word as carving's
 * shield does, but into a bitmap of one bit per slot and pose that the context owns; it grows only when the table does.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The entry point lives in a library of its own beside the module, libvgicp_hip_map_rays.so,
 * which links against libvgicp_hip.so and must come from the same build (a context of another build is refused).
 * VGICP_ABI_VERSION is unchanged, and no vgicp_set_option number is introduced. */
#ifndef VGICP_HIP_MAP_RAYS_H_
#define VGICP_HIP_MAP_RAYS_H_

#include "vgicp_hip.h"
#include "vgicp_hip_map_carve.h"   /* VGICP_CARVE_MAX_STEPS: the bound of a ray's walk is carving's */

#ifdef __cplusplus
extern "C" {
#endif

#define VGICP_RAYS_MAX_POSES 64

enum {
  VGICP_RAY_NO_RAY = 0,
  VGICP_RAY_OPEN = 1,
  VGICP_RAY_OWN = 2,
  VGICP_RAY_BEHIND = 3,
  VGICP_RAY_CONFIRMED = 4,
  VGICP_RAY_BLOCKED = 5,
  VGICP_RAY_NEAR = 6
};

typedef struct vgicp_ray_params {   /* 56 bytes, LP64 */
  double   origin[3];   /* the sensor's origin in the scan's frame (vgicp_carve_params.origin) */
  double   margin;      /* metres in front of its return within which a HIT is NEAR, not BLOCKED: finite, >= 0 */
  double   beyond;      /* metres a ray is followed behind its return: finite, >= 0 */
  double   max_range;   /* metres a ray is followed at most: finite, > 0, at most VGICP_CARVE_MAX_STEPS voxel sizes */
  uint32_t stride;      /* every stride-th point casts a ray: >= 1 */
  uint32_t reserved;    /* 0 */
} vgicp_ray_params;

typedef struct vgicp_ray_outputs {   /* 32 bytes, LP64: each plane optional, room for the resident scan's n points */
  uint8_t*  status;
  double*   range;
  int32_t*  hit_key;    /* 3 per point */
  uint32_t* steps;
} vgicp_ray_outputs;

typedef struct vgicp_ray_counts {   /* 80 bytes, LP64 */
  uint64_t rays;          /* rays cast */
  uint64_t visits;        /* voxels visited, over all rays */
  uint64_t by_class[8];   /* points per class; [0] the points without a ray, [7] zero */
} vgicp_ray_counts;

typedef struct vgicp_ray_stats {   /* 24 bytes, LP64 */
  int32_t launches, groups;           /* launches == 2 * groups */
  double  seconds, device_seconds;    /* host wall time of the call; event span around its groups */
} vgicp_ray_stats;

/* The ray report of the resident scan at n_poses poses (16 doubles each, as every transform of this ABI).  per_point
 * (optional): the planes, for a single pose only.  counts (optional): n_poses of them.  stats is optional.
 *
 * REFUSALS, in this order; VGICP_ERR_BAD_ARGUMENT unless stated.  A refused call writes nothing: not to the map, not to
 * the scan, not to the planes, counts or *stats:
 *   1. NULL ctx;
 *   2. a context that was not made by this build of the module;
 *   3. no map, or no resident scan (VGICP_ERR_NOT_READY);
 *   4. NULL poses or params, or n_poses of 0 or above VGICP_RAYS_MAX_POSES;
 *   5. a pose or origin entry that is not finite;
 *   6. margin NaN, negative or infinite;
 *   7. beyond NaN, negative or infinite;
 *   8. max_range not finite or <= 0, or max_range / voxel_size > VGICP_CARVE_MAX_STEPS;
 *   9. stride == 0 or reserved != 0;
 *  10. per-point outputs requested with n_poses != 1;
 *  11. a multi-device context (vgicp_create_multi), a communicator or a peer-connected context, with a text in
 *      vgicp_last_error.
 *
 * An empty scan returns VGICP_OK with zero counts and no launch; an empty map makes every ray OPEN.
 *
 * POSES IN GROUPS.  A pose's bitmap is slots / 8 bytes; a group holds as many poses as fit 16 MiB of bitmaps, at least
 * one.  Per group: the bitmaps are cleared, then a CONFIRM launch and a WALK launch, each one lane per point and pose.
 * Every group goes on the context's stream with no host round trip between them.  Pending work is settled first; then
 * one host synchronisation of the call's own. */
int vgicp_rays_resident(vgicp_ctx* ctx, const double* poses /* n_poses x 16 */, size_t n_poses,
                        const vgicp_ray_params* params, const vgicp_ray_outputs* per_point /* optional; n_poses == 1 only */,
                        vgicp_ray_counts* counts /* optional, n_poses */, vgicp_ray_stats* stats /* optional */);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_RAYS_H_ */
