/* vgicp_hip_map_submap.h — extension of the C ABI (vgicp_hip.h): SUBMAP AS SCAN.  The resident scan of a context made from
 * a region of a voxel map, on the device.
 *
 * Every registration entry point answers "where is this sweep in this map?".  Loop closure, the merge of a second session
 * into a first and the re-entry into a loaded map with more evidence than one sweep ask "where is this piece of map in
 * that map?".  A voxel record is a mean, a covariance and a count, which is what a VGICP source point is.  This call
 * turns the voxels of a region of `src`'s map (or of one of its levels, vgicp_hip_map_levels.h) into `dst`'s resident
 * scan, so that every resident call — vgicp_align_resident, _batch, _levels, vgicp_locate_resident,
 * vgicp_evaluate_resident, the reports, the insertions — becomes a map-to-map call.  No byte crosses the host.
 *
 * THE RULE, operation by operation (the kernels in vgicp_mapupdate.hip and tests/map_submap_reference.py restate it; IEEE
 * double arithmetic with NO fused multiply-add, every product and sum rounded once).
 *
 *   h           = voxel_size * 2^level, exact: the voxel size of the source table (level 0 is the map itself)
 *   SELECTION.  A FULL record with key K = (kx, ky, kz) and count c is selected iff vgicp_map_evict at `center` with
 *       distance_threshold = radius would KEEP it, and c >= min_count (min_count 0 and 1 select every count):
 *         d_a  = ((double)k_a + 0.5) * h - center_a                      per axis
 *         far  = sqrt((dx * dx + dy * dy) + dz * dz) > radius            LocalMap::needsPointRemoval
 *         selected = !far && (min_count <= 1 || c >= min_count)
 *       so a voxel whose centre lies exactly at distance radius is selected, and radius = +infinity selects by the
 *       count alone.  Tombstones and empty slots are never selected.  The device function that decides `far` is the
 *       one eviction runs.
 *   TRANSFORM.  frame = (R, t), column-major 4 x 4 as every pose of this ABI.  Selected voxel j becomes scan point j:
 *         point      = ((R[.,0] m0 + R[.,1] m1) + R[.,2] m2) + t         per row: the insertion's transform of a point
 *         RC         = (R[r,0] C[0,c] + R[r,1] C[1,c]) + R[r,2] C[2,c]   per entry
 *         covariance = (RC[r,0] R[c,0] + RC[r,1] R[c,1]) + RC[r,2] R[c,2]   i.e. (R C) R^T as the insertion rotates one
 *       With the identity frame a point and a covariance are the stored mean and covariance (x * 1 + 0 + 0 + 0).
 *   ORDER.  Points appear in ascending slot index of the source table.  The compaction is a prefix sum, not an atomic
 *       append: two calls on an unchanged map give byte-identical scans (and bit-identical aligns), and so do two
 *       contexts brought to the same map by the same sequence of calls, as far as their tables hold the keys in the
 *       same slots (keys that collide inside ONE batch race for their slots: the table's property, not this call's).
 *
 * WHAT THE CALL LEAVES IN dst.  Both layouts of the resident scan are written (the AoS copy and the twelve planes); the
 * scan counts as one whose covariances' symmetry is unknown (all twelve planes are read); the scan generation counter
 * advances by one; everything else is as after vgicp_scan_upload of the same points: vgicp_scan_info answers (n, 0, 0),
 * a fetch that was open and its checksums are void, and what is pending in dst is settled first — a preparation's
 * refusal that is still pending there is reported by this call, which then does nothing else.  When nothing is selected the call
 * returns VGICP_OK with points == 0 and dst has NO resident scan afterwards: resident calls answer VGICP_ERR_NOT_READY.
 * The key and the count of every selected voxel, in scan order, stay in device memory of dst;
 * vgicp_scan_from_map_keys delivers them while the scan generation is still the one the call produced.
 * src may be dst.  src's map, scan and scan generation are not touched (unless it is dst); dst's map never is.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The entry points live in a library of their own beside the module,
 * libvgicp_hip_map_submap.so, which links against libvgicp_hip.so and must come from the same build (a context of another
 * build is refused).  VGICP_ABI_VERSION is unchanged, and no vgicp_set_option number is introduced.  Nothing of this
 * header is allocated before the first call.  Single device; no asynchronous form: the selected count is needed on the
 * host before the next call can be planned. */
#ifndef VGICP_HIP_MAP_SUBMAP_H_
#define VGICP_HIP_MAP_SUBMAP_H_

#include "vgicp_hip.h"
#include "vgicp_hip_map_levels.h"   /* VGICP_LEVELS_MAX: `level` is one of the source's levels */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vgicp_submap_params {   /* 176 bytes, LP64 */
  double   center[3];   /* in the SOURCE map's frame */
  double   radius;      /* >= 0, or +infinity: the whole map */
  double   frame[16];   /* rigid transform applied to every selected voxel, column-major like every pose here */
  uint64_t min_count;   /* voxels with count < min_count are left out; 0 and 1 select every voxel */
  int32_t  level;       /* 0: the map; 1..4: that level of the source (vgicp_hip_map_levels.h) */
  int32_t  reserved;    /* 0 */
} vgicp_submap_params;

typedef struct vgicp_submap_stats {   /* 56 bytes, LP64 */
  uint64_t voxels;      /* FULL records of the source table looked at */
  uint64_t points;      /* selected = the size of dst's resident scan now */
  uint64_t too_far, too_few;   /* left out by the radius; by min_count among those inside the radius */
  int32_t  launches, reserved; /* kernel launches of this call: 3, and 2 per level it rebuilt; 0 */
  double   seconds, device_seconds;   /* host wall time of the call; event span around its launches */
} vgicp_submap_stats;

/* The resident scan of dst becomes the selected voxels of src's map.  stats is optional.
 *
 * REFUSALS, in this order; VGICP_ERR_BAD_ARGUMENT unless stated.  A refused call changes nothing in either context:
 *   1. NULL dst, src or params;
 *   2. dst or src was not made by this build of the module;
 *   3. dst or src is a multi-device context (vgicp_create_multi), has a communicator or is peer-connected;
 *   4. dst and src are on different devices;
 *   5. reserved != 0;
 *   6. level not 0 .. VGICP_LEVELS_MAX;
 *   7. level above the number of levels src was asked for (VGICP_ERR_NOT_READY): call vgicp_map_levels_build first;
 *   8. an entry of center or frame that is not finite;
 *   9. radius NaN, negative or -infinity;
 *  10. src has no map (VGICP_ERR_NOT_READY);
 *  11. once what is pending in both contexts has been settled: the source table holds more voxels than a resident scan
 *      may hold (the limit of vgicp_scan_upload).
 *
 * LAUNCHES, all on dst's stream behind an event of src's, with no host round trip between them and ONE host
 * synchronisation at the end, which brings the four counts.  MARK: one lane per slot reads the record's key and state
 * (its count where FULL and min_count asks), decides in registers; a wave stores its 64-bit ballot, a workgroup its
 * three counts.  SCAN: one workgroup takes the exclusive prefix sum over the workgroups' selected counts and the totals.
 * EMIT: a wave re-reads its ballot (a zero ballot touches no table line); a lane's rank is the workgroup's offset, the
 * popcounts of the ballots before its own and the bits below its own; selected lanes read the record, transform it and
 * write both layouts, the key and the count at that rank.  No workgroup waits for another. */
int vgicp_scan_from_map(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_submap_params* params,
                        vgicp_submap_stats* stats /* optional */);

/* The keys (n x 3) and counts (n) of the voxels that make up dst's resident scan, in scan order; each array optional.
 * *written = n.  VGICP_ERR_BAD_ARGUMENT: NULL dst or written, a context of another build, a multi-device context;
 * VGICP_ERR_NOT_READY: the resident scan is not (or no longer) the one vgicp_scan_from_map made;
 * VGICP_ERR_BAD_ARGUMENT with *written = n and nothing copied: capacity below n. */
int vgicp_scan_from_map_keys(vgicp_ctx* dst, size_t capacity, int32_t* keys /* n x 3, optional */,
                             uint64_t* counts /* n, optional */, size_t* written);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_SUBMAP_H_ */
