/* vgicp_hip_points.h — extension of the C ABI (vgicp_hip.h): the resident scan at a pose, point by point.
 *
 * Everything else the module reports about a registration is a sum over the scan: an align returns counts and normal
 * equations per round, vgicp_evaluate_resident a count, the objective and the squared error per pose.  This call says
 * what a single point contributes at a pose — matched or not, |e|^2, the squared Mahalanobis residual d^2 the robust
 * rounds of vgicp_hip_robust.h weight and gate by, and the weight the context's current robust options give it — and
 * order statistics of d^2, from which a scale and a gate are chosen in the library's own (regularised) units.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is what
 * libvgicp_hip.so exports.  The entry point lives in a library of its own beside the module, libvgicp_hip_points.so,
 * which links against libvgicp_hip.so and must come from the same build (a context of another build is refused).
 * VGICP_ABI_VERSION is unchanged, and no vgicp_set_option number is introduced. */
#ifndef VGICP_HIP_POINTS_H_
#define VGICP_HIP_POINTS_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VGICP_POINT_QUANTILES_MAX 16
#define VGICP_POINT_MATCHED    1u  /* the point's voxel is in the map at this pose */
#define VGICP_POINT_NEGATIVE   2u  /* matched, raw e^T W e < 0 (an indefinite covariance) */
#define VGICP_POINT_NOT_FINITE 4u  /* matched, raw e^T W e is NaN or +-inf */

typedef struct vgicp_point_summary {   /* 168 bytes, LP64 */
  uint64_t points;      /* n of the resident scan */
  uint64_t matched;     /* == vgicp_evaluation.correspondences at this pose */
  uint64_t counted;     /* weight > 0 under the context's robust options */
  uint64_t negative;
  uint64_t not_finite;
  double   quantile[VGICP_POINT_QUANTILES_MAX];
} vgicp_point_summary;

typedef struct vgicp_point_stats {
  int32_t launches;        /* kernel launches of the call: 2, plus the sort's (1 + merge levels) when quantiles are asked */
  int32_t reserved;
  double  seconds;         /* host wall time of the call */
  double  device_seconds;  /* event span around the launches of the call (the copies of the arrays follow it) */
} vgicp_point_stats;

/* The resident scan at `pose` (16 doubles, laid out as vgicp_align_resident's guess), point by point.
 *
 * PER POINT i of the resident scan.  e = R p + t - mu_voxel, W = (R C R^T + C_voxel)^-1 and raw = e^T W e are formed as
 * every round and vgicp_evaluate_resident form them (the exact-voxel lookup, the cofactor inverse, W e first and then
 * e . (W e)).
 *   matched      d2[i] = raw (it may be negative or NaN: the flags say so), sq_error[i] = |e|^2, weight[i] = the weight
 *                a robust round gives the correspondence under the context's current VGICP_OPTION_ROBUST_KERNEL,
 *                _SCALE_MICRO and _GATE_MICRO (1.0 with all three at their defaults), status[i] = VGICP_POINT_MATCHED,
 *                plus VGICP_POINT_NOT_FINITE when raw is NaN or infinite, else plus VGICP_POINT_NEGATIVE when raw < 0.
 *   not matched  d2[i] = sq_error[i] = +infinity, weight[i] = 0, status[i] = 0.
 * So d2[i] <= g is exactly "a round gated at g counts this point", for every point of the scan.
 * Each of the four arrays may be NULL; those given hold `capacity` entries, and the first n are written.
 *
 * SUMMARY (may be NULL unless quantiles are asked).  points, matched, negative, not_finite count the points and the
 * flags; counted is the number of points with weight > 0: corr_count[0] of a robust vgicp_align_resident from this pose.
 * quantile[j], j < n_quantiles, is an ORDER STATISTIC of d^2, never interpolated: of the m points that are matched and
 * not VGICP_POINT_NOT_FINITE, each ranked by max(raw, 0) (the d^2 the weights use), the value of rank
 *     min(max(ceil(q[j] * m), 1), m) - 1
 * in ascending order, the expression evaluated in fp64.  m = 0 gives NaN for every quantile.  Entries of quantile[] from
 * n_quantiles on are not written.
 *
 * REFUSALS, in this order; VGICP_ERR_BAD_ARGUMENT unless stated, and nothing is written except where stated:
 *    1. NULL ctx;
 *    2. a context that was not made by this build of the module;
 *    3. NULL pose;
 *    4. a pose entry that is not finite;
 *    5. n_quantiles > VGICP_POINT_QUANTILES_MAX;
 *    6. n_quantiles > 0 with q or summary NULL;
 *    7. a q[j] outside [0, 1] or NaN;
 *    8. a multi-device context (vgicp_create_multi), a communicator or a peer-connected context (the resident scan of a
 *       device is a shard there), with a text in vgicp_last_error;
 *    9. no map, or no resident scan: VGICP_ERR_NOT_READY;
 *   10. after settling, any of the four arrays given with capacity < n: summary->points is set (when summary is given),
 *       so the caller can size its arrays and call again.
 * All four arrays NULL, n_quantiles == 0 and a summary is allowed: it returns the five counts.
 *
 * A scan that is still pending (after vgicp_scan_prepare_async) and a pending map insertion are settled first, as
 * vgicp_evaluate_resident settles them.
 *
 * READ-ONLY, in vgicp_evaluate_resident's sense.  The scan generation counter does not move; nothing is written to the
 * map, the resident scan, the memo of the launch-per-round loop, the exchange buffers of the persistent launch or the
 * cool-down; VGICP_COUNTER_PERSISTENT_FALLBACKS cannot move.  An align, a batch or an evaluation after this call returns
 * the bits it returns without it.
 *
 * INDEPENDENCE.  What is reported for a point does not depend on which outputs were asked for, on the quantiles, or on
 * the points behind it in the scan; two calls return the same bits.
 *
 * ONE host synchronisation per call (besides the one that settles pending work).  One launch forms the per-point values
 * (one lookup per point; nothing in it waits for another workgroup), the library's own sort orders the 64-bit patterns
 * of max(raw, 0) when quantiles are asked, and one small launch picks the ranks on the device and writes quantiles and
 * counts into page-locked memory of the context.  The arrays travel through the context's page-locked arena, as
 * vgicp_scan_download's do: the runtime never sees the caller's pages.  Device scratch (57 bytes per point of the scan's
 * capacity) is allocated by the first call and grows only: calls on scans of one size allocate once. */
int vgicp_points_resident(vgicp_ctx* ctx, const double pose[16], size_t capacity,
                          double* d2, double* sq_error, double* weight, uint8_t* status, /* each optional, capacity entries */
                          size_t n_quantiles, const double* q,                           /* optional */
                          vgicp_point_summary* summary, vgicp_point_stats* stats);       /* each optional */

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_POINTS_H_ */
