/* vgicp_hip_map_gated.h — extension of the C ABI (vgicp_hip.h): insert the resident scan into the map WITHOUT the points
 * a gate on the squared Mahalanobis residual rejects.
 *
 * vgicp_map_insert_resident and its _async form insert every point of the scan.  A moving object that the robust rounds
 * of vgicp_hip_robust.h ignored is then averaged into the voxels it passed through, and the next frame registers
 * against that.  The calls below evaluate every point against the map as it stands BEFORE the call, exactly as
 * vgicp_points_resident of vgicp_hip_points.h reports it, and insert only the points the gate lets through — on the
 * device, in the stream, without the scan ever visiting the host.
 *
 * THE RULE.  Point i of the resident scan is REFUSED iff vgicp_points_resident at the pose `transform` would report it
 * VGICP_POINT_MATCHED and not max(d2[i], 0) <= gate.  So
 *   - a matched point with VGICP_POINT_NOT_FINITE is refused at every gate, +infinity included;
 *   - a VGICP_POINT_NEGATIVE point counts as d^2 = 0 and is kept;
 *   - a point that is not matched opens new ground and is kept.
 * The kept points are inserted in scan order exactly as vgicp_map_insert_resident inserts a scan that holds only them:
 * the same arithmetic, the same order inside a voxel, the same ordinals in the raw-point store (vgicp_hip_map_points.h).
 * "Matched" is "the voxel this point would be inserted into exists already": a refused point never creates a voxel.
 *
 * UNITS.  `gate` is in the library's regularised units: those of VGICP_OPTION_ROBUST_GATE_MICRO / 1e6, of the d2[] and
 * the quantiles of vgicp_points_resident, and of ICP::robustScaleFromQuantile in the shim.  It is finite and >= 0, or
 * +infinity (only what is not finite is refused).  The context's robust options play no part in the decision.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The three entry points live in a library of their own beside the module,
 * libvgicp_hip_map_gated.so, which links against libvgicp_hip.so and must come from the same build (a context of
 * another build is refused).  VGICP_ABI_VERSION is unchanged, and no vgicp_set_option number is introduced. */
#ifndef VGICP_HIP_MAP_GATED_H_
#define VGICP_HIP_MAP_GATED_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vgicp_gated_insert_stats {   /* 64 bytes, LP64 */
  uint64_t points, matched, refused, not_finite;  /* of this call; points - refused were offered to the map */
  uint64_t new_voxels;
  int32_t  launches, reserved;
  double   seconds, device_seconds;   /* host wall time of the call; event span around its launches */
} vgicp_gated_insert_stats;

/* The gated form of vgicp_map_insert_resident.  kept (optional, `capacity` entries): 1 where point i was kept, 0 where it
 * was refused; the first n are written.  stats is optional.
 *
 * REFUSALS, in this order; VGICP_ERR_BAD_ARGUMENT unless stated.  A refused call writes nothing to the map, the
 * raw-point store or the scan, and the scan generation counter does not move:
 *   1. NULL ctx;
 *   2. a context that was not made by this build of the module;
 *   3. everything vgicp_map_insert_resident refuses, in its order (no map and no resident scan: VGICP_ERR_NOT_READY);
 *   4. a transform entry that is not finite;
 *   5. a gate that is NaN, negative or -infinity;
 *   6. a multi-device context (vgicp_create_multi), a communicator or a peer-connected context, with a text in
 *      vgicp_last_error;
 *   7. after settling, kept given with capacity < n: stats->points is set (when stats is given), so the caller can size
 *      the array and call again.
 *
 * TWO STEPS on the context's stream, never fused.  The decision is one read-only launch (one lookup per point, the term
 * of vgicp_points_resident by the same device function, nothing in it waits); the insertion is
 * vgicp_map_insert_resident's own launches, whose first skips the refused points: no probe, no claim, and not counted as
 * "table full".  A slot that the insertion is claiming is therefore never something the decision can see.
 * One host synchronisation (besides the one that settles pending work, and a table or store that has to grow). */
int vgicp_map_insert_resident_gated(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel, double gate,
                                    size_t capacity, uint8_t* kept /* optional: 1 kept, 0 refused, first n written */,
                                    vgicp_gated_insert_stats* stats /* optional */);

/* The gated form of vgicp_map_insert_resident_async: settles what that call settles, waits for nothing else, refuses by
 * rules 1 to 6 above.  Its counts are added to running totals on the device, which the next synchronisation of the
 * context reads with the insertion's own; until then the host counts every point of the scan as possibly inserted. */
int vgicp_map_insert_resident_gated_async(vgicp_ctx* ctx, const double transform[16], size_t max_points_per_voxel,
                                          double gate);

/* Points that the gated calls of this context saw and refused since the last vgicp_map_reset; either may be NULL.
 * Settles pending work first.  Refuses by rules 1 and 2. */
int vgicp_map_gated_totals(vgicp_ctx* ctx, uint64_t* points, uint64_t* refused);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_MAP_GATED_H_ */
