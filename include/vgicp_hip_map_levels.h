/* vgicp_hip_map_levels.h — extension of the C ABI (vgicp_hip.h): MAP LEVELS.  The voxel map again at 2, 4, 8 and 16 times
 * its voxel size, kept on the device, and an align that walks through them.
 *
 * Every registration entry point matches a scan point to the one voxel it falls into, so an align converges from about
 * one voxel away.  A level is the same map with voxels twice as wide as the level below; an align against level 3 of a
 * 0.3 m map converges from 1.2 m away and leaves a pose that level 2 converges from, and so on down to the map itself.
 *
 * THE RULE, operation by operation (the kernels in vgicp_levels.hip and tests/map_levels_reference.py restate it; IEEE
 * double arithmetic with NO fused multiply-add, every product, sum and quotient rounded once).  Level 0 is the map.
 * Level l >= 1 has voxel size voxel_size * 2^l and is derived from level l-1 alone:
 *
 *   a level-l voxel exists for every key K = k >> 1, k the key of a FULL voxel of level l-1; the shift is an
 *       arithmetic shift per component (-1 -> -1).  Tombstones and empty slots are nobody's children;
 *   its children are the up to eight FULL voxels 2K + (dx, dy, dz) of level l-1, dx, dy, dz in {0, 1}, taken in
 *       OCTANT ORDER o = dx + 2 dy + 4 dz;
 *   with exactly one child, mean, covariance and count are the child's, bit for bit;
 *   with more than one child,
 *       N = sum of count_c                                         (integers)
 *       mean[e] = (sum_c (double)count_c * mean_c[e]) / (double)N  for each of the three entries
 *       cov[e]  = (sum_c (double)count_c * cov_c[e])  / (double)N  for each of the nine entries
 *       the sums run over the children in octant order and start from the first child's product;
 *   count = N (it is not frozen at any cap).
 *
 * For a map in which no voxel has reached its cap, this is, up to rounding, the voxel the running mean of
 * vgicp_map_insert_* would hold at that size.  Because the size changes by a power of two,
 * floor(fl(x / (h 2^l))) == floor(fl(x / h)) >> l holds exactly wherever the quotient does not underflow: a level is
 * addressed by the map's own key function at the level's voxel size.  (The exception: a negative coordinate within
 * 2^-1074 h 2^l of 0, some 1e-323 m, has the map key -1 and the level key 0; tests/test_map_levels_cpu.py pins it.)
 *
 * LAZINESS.  The context keeps the number of levels asked for (0 after vgicp_create: nothing of this header is allocated
 * or run) and the map's version each level was built at.  Every call below that reads a level first settles what is
 * pending on the context and then rebuilds the levels that are out of date — never when the map has not changed since.
 * A rebuild is whole (two launches per level, CLAIM and FILL, no host round trip between levels).  vgicp_map_reset keeps
 * the number and empties the levels.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The four entry points live in a library of their own beside the module,
 * libvgicp_hip_map_levels.so, which links against libvgicp_hip.so and must come from the same build (a context of
 * another build is refused).  VGICP_ABI_VERSION is unchanged, and no vgicp_set_option number is introduced.
 *
 * REFUSALS of the four calls, in this order; VGICP_ERR_BAD_ARGUMENT unless stated.  A refused call writes nothing:
 *   1. NULL ctx (or a context that was not made by this build of the module), or a NULL pointer that is not optional;
 *   2. `levels` not 0 .. VGICP_LEVELS_MAX; `level` or a stage's level not 0 .. VGICP_LEVELS_MAX; `stages` not
 *      1 .. VGICP_LEVEL_STAGES_MAX;
 *   3. `level` or a stage's level above the number of levels asked for (VGICP_ERR_NOT_READY);
 *   4. an entry of `guess` that is not finite;
 *   5. a stage's params that vgicp_align_resident refuses (max_iteration < 0);
 *   6. a multi-device context (vgicp_create_multi), a communicator or a peer-connected context;
 *   7. no map; for vgicp_align_resident_levels also no resident scan (VGICP_ERR_NOT_READY);
 *   8. vgicp_map_level_export with something to write and a NULL array. */
#ifndef VGICP_HIP_MAP_LEVELS_H_
#define VGICP_HIP_MAP_LEVELS_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VGICP_LEVELS_MAX 4
#define VGICP_LEVEL_STAGES_MAX 8

typedef struct vgicp_levels_stats {   /* 104 bytes, LP64 */
  uint64_t voxels[VGICP_LEVELS_MAX + 1];   /* [l]: voxels of level l, [0] the map's; 0 above `levels` */
  uint64_t slots[VGICP_LEVELS_MAX + 1];    /* [l]: slots of level l's table */
  int32_t  levels;                         /* the number of levels asked for */
  int32_t  launches;                       /* kernel launches of this call: 2 per level it rebuilt */
  double   seconds, device_seconds;        /* host wall time of the call; event span around its launches */
} vgicp_levels_stats;

/* Ask for `levels` levels (0 .. VGICP_LEVELS_MAX) and bring them up to date now; 0 releases every level's storage.
 * Levels that are up to date already are not rebuilt (launches then says so).  stats is optional.  One host
 * synchronisation. */
int vgicp_map_levels_build(vgicp_ctx* ctx, int levels, vgicp_levels_stats* stats /* optional */);

/* Voxels, table slots and voxel size of a level (0: the map itself); each output is optional. */
int vgicp_map_level_size(vgicp_ctx* ctx, int level, size_t* voxels, size_t* table_slots, double* voxel_size);

/* A level's voxels as vgicp_map_export gives the map's (order unspecified); level 0 IS vgicp_map_export. */
int vgicp_map_level_export(vgicp_ctx* ctx, int level, size_t capacity, int32_t* keys, double* means, double* covs,
                           uint64_t* counts, size_t* written);

/* Register the resident scan in `stages` stages: stage i is vgicp_align_resident against level levels[i] with params[i],
 * started from the pose the stage before it returned (stage 0: from `guess`): the same plan, the same launches and the
 * same fallback as vgicp_align_resident, over that level's table and voxel size; the robust round and the pose prior
 * apply as they are set.  The sequence of levels is free: it need not descend or end at 0.  One host synchronisation
 * per stage.  stats: NULL, or `stages` blocks, each filled as vgicp_align_resident fills its one.  A stage that fails ends
 * the call with that stage's status; out_pose then holds nothing. */
int vgicp_align_resident_levels(vgicp_ctx* ctx, const double guess[16], size_t stages, const int32_t* levels,
                                const vgicp_params* params /* stages */, double out_pose[16],
                                vgicp_stats* stats /* stages, may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_LEVELS_H_ */
