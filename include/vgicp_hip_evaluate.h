/* vgicp_hip_evaluate.h — extension of the C ABI (vgicp_hip.h): how good is a pose?  Fitness, inlier RMSE and the VGICP
 * objective of the resident scan at several poses, in one launch pair.
 *
 * An align reports the correspondence count and the normal equations of each round, which describe the pose BEFORE that
 * round's step; nothing scores the pose that is returned.  vgicp_evaluate_resident evaluates any k poses of the resident
 * scan against the map — the returned pose of an align, the k poses of vgicp_align_resident_batch, a prior — and
 * reports, per pose, what an Open3D-style registration result carries (fitness = correspondences / points,
 * inlier_rmse = sqrt(sq_error / correspondences)), the objective ICP::align minimises, and the normal equations at that
 * pose (J^T S^-1 J is the information matrix of the pose).  The correspondence rule is the reference's exact-voxel
 * lookup (LocalMap::correspondenceMatching, src/LocalMap.cpp:78-112).
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned.  The function is defined in
 * the same library (libvgicp_hip.so); VGICP_ABI_VERSION is unchanged. */
#ifndef VGICP_HIP_EVALUATE_H_
#define VGICP_HIP_EVALUATE_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VGICP_EVAL_MAX 64 /* poses per call */

typedef struct vgicp_evaluation {      /* 248 bytes, LP64 */
  uint64_t points;           /* n of the resident scan */
  uint64_t correspondences;  /* points whose voxel is in the map at this pose */
  double   cost;             /* sum over correspondences of e^T (R C R^T + C_voxel)^-1 e, e = R p + t - mean */
  double   sq_error;         /* sum over correspondences of |e|^2 */
  double   normal_eq[27];    /* 21 lower-triangle J^T S^-1 J + 6 J^T S^-1 r, laid out as in vgicp_stats */
} vgicp_evaluation;

typedef struct vgicp_eval_stats {
  int32_t launches;          /* kernel launches of the call: two per group of poses_per_launch poses */
  int32_t poses_per_launch;  /* how many poses one launch pair takes for the scan that is resident now */
  double  seconds;           /* host wall time of the call */
  double  device_seconds;    /* event span around all launches of the call */
} vgicp_eval_stats;

/* Evaluates the resident scan at k poses (k x 16 doubles, each laid out as vgicp_align_resident's guess); out receives
 * k evaluations.  stats may be NULL.
 *
 * 1 <= k <= VGICP_EVAL_MAX, else VGICP_ERR_BAD_ARGUMENT.  NULL poses or out: VGICP_ERR_BAD_ARGUMENT.  A pose with an
 * entry that is not finite: VGICP_ERR_BAD_ARGUMENT — checked on the host for all k poses before anything is launched,
 * and nothing is written to out.  VGICP_ERR_NOT_READY without a map or a resident scan.  A scan that is still pending
 * (after vgicp_scan_prepare_async) and a pending map insertion are settled first, as vgicp_align_resident_batch settles
 * them (the launch geometry is made from the kept count).
 *
 * READ-ONLY.  The scan generation counter does not move; nothing is written to the map, the resident scan, the memo of
 * the launch-per-round loop (the kernels take none), the exchange buffers of the persistent launch and their rotation,
 * the batch's exchange words or the cool-down; VGICP_COUNTER_PERSISTENT_FALLBACKS cannot move.  A vgicp_align_resident
 * or a vgicp_align_resident_batch after an evaluation returns the bits it returns without one.
 *
 * BIT EQUALITY.  For every scan size, correspondences and normal_eq of pose h are bit for bit what the
 * launch-per-round loop produces for round 0 with that pose as the guess: corr_count[0] and row 0 of normal_eq of
 * vgicp_align_resident with VGICP_FLAG_NO_PERSISTENT, and what vgicp_accumulate returns on the same scan; for scans of
 * at most grid x 448 points (grid = min(compute units, 256)) therefore also row 0 of the persistent launch and of a
 * batch.  The summation order is that of the loop's 512-thread launch: min(ceil(n / 448), 512) workgroups per pose whose
 * waves 1-7 own the points, grid-stride; inside a wave a 32-slot halving butterfly, then the waves pairwise, then the
 * workgroups' rows as pairwise trees of 16 (rows that belong to no workgroup count as +0.0 in their place of the tree).
 * cost and sq_error travel through the same sums in two spare slots of the 32-double row: they are reproducible bit for
 * bit from run to run, and the evaluation of a pose does not depend on k, on the pose's position in the call or on its
 * neighbours.
 *
 * ONE host synchronisation per call.  The k poses run in as few launch pairs (evaluate, fold) as a fixed budget of
 * 4 096 partial rows allows: poses_per_launch = min(VGICP_EVAL_MAX, floor(4 096 / rows per pose)), at least 16 for
 * scans of up to 256 x 448 points and 8 beyond.  Poses reach the device and results come back through page-locked
 * memory; no copy is enqueued.
 *
 * Nothing is allocated inside the call, on the device or page-locked: the rows (1 MiB on the device), the poses and the
 * results (22 KB page-locked) are made by vgicp_create.
 *
 * Every wait is bounded because there is none: the kernels contain no poll, no flag and no wait for another workgroup;
 * kernel boundaries are the only grid-wide synchronisation, so there is no give-up path and no fallback.
 *
 * Not available on multi-device contexts (vgicp_create_multi), communicators and peer-connected contexts (the resident
 * scan of a device is a shard there): VGICP_ERR_BAD_ARGUMENT, with a text in vgicp_last_error. */
int vgicp_evaluate_resident(vgicp_ctx* ctx, size_t k, const double* poses /* k x 16 */, vgicp_evaluation* out /* k */,
                            vgicp_eval_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_EVALUATE_H_ */
