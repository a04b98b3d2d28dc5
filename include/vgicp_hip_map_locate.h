/* vgicp_hip_map_locate.h — extension of the C ABI (vgicp_hip.h): LOCATE.  Up to 64 poses of the resident scan scored over
 * a window of whole-voxel shifts on a level of the map (include/vgicp_hip_map_levels.h), read-only.
 *
 * Every registration entry point converges from about one voxel of the level it runs against: the chain 3 -> 2 -> 1 -> 0 of
 * vgicp_align_resident_levels on a 0.3 m map from about 1.2 m.  The first frame against a loaded map, a frame after a
 * stall and a re-entry after the filter has drifted by metres have no such guess.  On level l a translation by a whole
 * voxel of that level is an integer shift of a point's key, so ONE transform of a point serves every translation of a
 * window, and the score of a translation is an integer: how many scan points land in a FULL voxel.  This is a correlative
 * search on the voxel hash; its result is the guess vgicp_align_resident_levels needs.
 *
 * THE RULE, operation by operation (the kernels in vgicp_levels.hip and tests/map_locate_reference.py restate it; IEEE
 * double arithmetic with NO fused multiply-add, every product, sum and quotient rounded once).  Inputs: the resident
 * scan of n points p_i in its own frame, k poses T = (R, t) and vgicp_locate_params.
 *
 *   h           = voxel_size * 2^level, exact: the level's voxel size (level 0 is the map itself)
 *   Only points with i % stride == 0 TAKE PART.
 *   e = T p     is the insertion's transform:  ((R[.,0] x0 + R[.,1] x1) + R[.,2] x2) + t   per row
 *   K = key(e)  is the insertion's key:        floor(e / h) per axis; DEFINED iff all three are within +-2^30
 *   A point that takes part whose e is not finite or whose key is not defined is SKIPPED, and counted as such.
 *   A CELL is a shift d = (dx, dy, dz) with |dx| <= wx, |dy| <= wy, |dz| <= wz, (wx, wy, wz) = window; its index is
 *       c = ((dz + wz) (2 wy + 1) + (dy + wy)) (2 wx + 1) + (dx + wx),     cells = (2 wx + 1)(2 wy + 1)(2 wz + 1)
 *   hits[pose][c] = the number of points i that take part and are not skipped for which the level holds a FULL voxel
 *       with the key K_i + d.  Tombstones and empty slots hit nothing.
 *
 * Per pose, vgicp_locate_best: the maximum of hits over the cells; `cell`, the LOWEST index that attains it; `offset`,
 * that cell's d; `points`, the points that took part and were not skipped; `skipped`; and `pose`, the input pose with
 *       t_a + (double)d_a * h     added per axis: one product and one sum, each rounded once.
 * That pose is a guess for an align.  The score itself is defined by the shift of the KEY, never by moving the point: a
 * point within rounding of a voxel face may have another key at the moved pose.
 *
 * Every sum is an integer, so nothing depends on the order in which the device counts: a call's result is the rule's,
 * exactly, and the same from run to run.
 *
 * READ-ONLY, as vgicp_rays_resident: the table's bytes do not change, the scan's generation counter does not move, the
 * map's version is not bumped, and no counter, memo or exchange word of an align moves: an align before and after the
 * call returns the same bits.  A level >= 1 is read through the levels' laziness: pending work is settled, a level that
 * is out of date is rebuilt, and never when the map has not changed since.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The entry point lives in a library of its own beside the module, libvgicp_hip_map_locate.so,
 * which links against libvgicp_hip.so and must come from the same build (a context of another build is refused).
 * VGICP_ABI_VERSION is unchanged, and no vgicp_set_option number is introduced.  Nothing of this header is allocated
 * before the first call. */
#ifndef VGICP_HIP_MAP_LOCATE_H_
#define VGICP_HIP_MAP_LOCATE_H_

#include "vgicp_hip.h"
#include "vgicp_hip_map_levels.h"   /* VGICP_LEVELS_MAX: `level` is one of the map's levels */

#ifdef __cplusplus
extern "C" {
#endif

#define VGICP_LOCATE_MAX_POSES 64
#define VGICP_LOCATE_MAX_HALF_WIDTH 32
#define VGICP_LOCATE_MAX_CELLS 4096

typedef struct vgicp_locate_params {   /* 20 bytes */
  int32_t  level;       /* 0 .. VGICP_LEVELS_MAX, at most the number of levels asked for */
  int32_t  window[3];   /* half-widths (wx, wy, wz) in voxels of the level: 0 .. VGICP_LOCATE_MAX_HALF_WIDTH each */
  uint32_t stride;      /* every stride-th point takes part: >= 1 */
} vgicp_locate_params;

typedef struct vgicp_locate_best {   /* 160 bytes, LP64 */
  uint32_t hits;        /* of the best cell */
  uint32_t cell;        /* the lowest index that attains `hits` */
  int32_t  offset[3];   /* that cell's shift d, in voxels of the level */
  uint32_t points;      /* points that took part and were not skipped */
  uint32_t skipped;
  uint32_t reserved;    /* 0 */
  double   pose[16];    /* the input pose with d * h added to its translation */
} vgicp_locate_best;

typedef struct vgicp_locate_stats {   /* 24 bytes, LP64 */
  int32_t cells;                      /* of the window */
  int32_t launches;                   /* kernel launches of this call: 2, and 2 per level it rebuilt */
  double  seconds, device_seconds;    /* host wall time of the call; event span around its launches */
} vgicp_locate_stats;

/* Score k poses (16 doubles each, as every transform of this ABI) of the resident scan over the window.  best: k of
 * them.  hits (optional): the whole plane, k x cells, pose-major.  stats is optional.
 *
 * REFUSALS, in this order; VGICP_ERR_BAD_ARGUMENT unless stated.  A refused call writes nothing: not to the map, not to
 * the scan, not to best, hits or *stats:
 *   1. NULL ctx (or a context that was not made by this build of the module); NULL poses, params or best;
 *   2. k not 1 .. VGICP_LOCATE_MAX_POSES; level not 0 .. VGICP_LEVELS_MAX; a half-width not
 *      0 .. VGICP_LOCATE_MAX_HALF_WIDTH; cells above VGICP_LOCATE_MAX_CELLS; stride == 0;
 *   3. level above the number of levels asked for (VGICP_ERR_NOT_READY): call vgicp_map_levels_build first;
 *   4. an entry of a pose that is not finite;
 *   5. a multi-device context (vgicp_create_multi), a communicator or a peer-connected context;
 *   6. no map, or no resident scan (VGICP_ERR_NOT_READY).
 *
 * An empty map scores zero everywhere: the best cell is then cell 0.
 *
 * LAUNCHES.  One clear of the plane; a SCORE launch over (pose, chunk of the points that take part), in which a
 * workgroup makes each point's key once, probes the level's table once per point and cell and counts in a histogram of
 * the window in its local memory; a BEST launch, one workgroup per pose, that writes vgicp_locate_best into page-locked
 * memory.  All on the context's stream with no host round trip between them; then one host synchronisation. */
int vgicp_locate_resident(vgicp_ctx* ctx, const double* poses /* k x 16 */, size_t k, const vgicp_locate_params* params,
                          vgicp_locate_best* best /* k */, uint32_t* hits /* optional, k x cells */,
                          vgicp_locate_stats* stats /* optional */);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_LOCATE_H_ */
