/* vgicp_hip_map_points.h — extension of the C ABI (vgicp_hip.h): the raw points of the device map.
 *
 * The reference's voxel keeps more than a mean and a covariance: Voxel::points holds the first maxNumPoints world-frame
 * points that reached it, in insertion order (include/ESKF_LIO/LocalMap.hpp:63-87, src/LocalMap.cpp:47-58), and
 * LocalMap::save() writes exactly those (src/LocalMap.cpp:156-167).  With VGICP_OPTION_MAP_RAW_POINTS on, the device
 * map keeps them too: every point an insertion ACCEPTS (the voxel's constructor, or addPoint while count < max) is
 * recorded as the insertion transformed it — vgicp_map_insert_scan, vgicp_map_insert_resident and
 * vgicp_map_insert_resident_async alike — at 32 bytes per point on the device.  Means, covariances and counts are the
 * same bits with the store on or off, and the resident frame chain keeps its one host synchronisation per frame
 * (the store grows, with a synchronisation, only when it could fill).
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned.  Both functions are defined
 * in the same library (libvgicp_hip.so). */
#ifndef VGICP_HIP_MAP_POINTS_H_
#define VGICP_HIP_MAP_POINTS_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Option of vgicp_set_option. value != 0: the map keeps its raw points (see above); 0: it does not (the default).
 * Accepted only while the map holds no voxel (after vgicp_create or vgicp_map_reset, or once every voxel has been
 * erased or evicted); otherwise VGICP_ERR_BAD_ARGUMENT.  While it is on:
 *   - vgicp_map_upsert returns VGICP_ERR_BAD_ARGUMENT (a mirror batch carries no raw points);
 *   - an insertion with max_points_per_voxel >= 2^32 returns VGICP_ERR_BAD_ARGUMENT;
 *   - vgicp_map_erase and vgicp_map_evict drop the points of the voxels they remove; a point that later falls into
 *     such a voxel starts a fresh list, as the reference's constructor does;
 *   - vgicp_map_reset empties the store (it stays on).
 * A multi-device context keeps the store on its first device only. */
#define VGICP_OPTION_MAP_RAW_POINTS 4

/* points: the raw points the map holds (the sum of the voxels' counts); capacity: the entries the device store can
 * hold before it has to grow (each live or dead: dead entries are reclaimed when it grows or the table rehashes).
 * Either pointer may be NULL.  Settles a pending insertion.  VGICP_ERR_NOT_READY while the store is off. */
int vgicp_map_points_size(const vgicp_ctx* ctx, size_t* points, size_t* capacity);

/* Writes one key (3 x int32) and one point (3 doubles, world frame) per raw point: every voxel's points contiguous and
 * in insertion order (Voxel::points), as many as its count; the order of the voxels is unspecified.  capacity in
 * points; `written` receives min(points, capacity) (a capacity below vgicp_map_points_size's count cuts the output
 * short).  Settles a pending insertion first, like vgicp_map_export.  VGICP_ERR_NOT_READY while the store is off. */
int vgicp_map_points_export(vgicp_ctx* ctx, size_t capacity, int32_t* keys, double* points, size_t* written);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_POINTS_H_ */
