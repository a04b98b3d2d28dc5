/* vgicp_hip_batch.h — extension of the C ABI (vgicp_hip.h): one resident scan registered from several initial guesses.
 *
 * The reference's frame loop registers one scan from one guess (src/ErrorStateKF.cpp:130).  An integrator that has no
 * prior yet, that comes out of a stall or a corridor, or that re-enters a map built earlier registers a small fan of
 * guesses around its prior and keeps the best.  vgicp_align_resident_batch does that in one call: on a single-device
 * context the hypotheses run side by side as TEAMS of workgroups inside ONE persistent launch (a scan of n points
 * occupies ceil(n / 448) of the launch's workgroups, the others would idle), with one host synchronisation.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned.  Both functions are defined
 * in the same library (libvgicp_hip.so); VGICP_ABI_VERSION is unchanged. */
#ifndef VGICP_HIP_BATCH_H_
#define VGICP_HIP_BATCH_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VGICP_BATCH_MAX 64 /* hypotheses per call */

typedef struct vgicp_batch_stats {
  int32_t hypotheses_per_launch;  /* how many shared a launch; 1 = they ran one after another */
  int32_t launches;
  double  seconds;                /* host wall time of the call */
  double  device_seconds;         /* event span around all launches of the call */
  int32_t*  status;      /* optional, k: VGICP_OK or VGICP_ERR_DEGENERATE per hypothesis */
  int32_t*  iterations;  /* optional, k */
  int32_t*  converged;   /* optional, k */
  uint64_t* corr_count;  /* optional, k x max_iteration */
  double*   normal_eq;   /* optional, k x max_iteration x 27, laid out as in vgicp_stats */
} vgicp_batch_stats;

/* Registers the resident scan against the map from k guesses (k x 16 doubles, each laid out as vgicp_align_resident's
 * guess); out_poses receives k poses.  stats may be NULL, and so may each of its arrays.
 *
 * For every h the pose, iterations[h], converged[h], the first iterations[h] entries of corr_count + h * max_iteration
 * and the first iterations[h] rows of normal_eq + h * max_iteration * 27 are BIT FOR BIT what
 * vgicp_align_resident returns for the guess at guesses + 16 * h on the same context state: a hypothesis does not
 * depend on its neighbours, on its position in the batch or on k.
 *
 * 1 <= k <= VGICP_BATCH_MAX, else VGICP_ERR_BAD_ARGUMENT.  VGICP_ERR_NOT_READY without a map or a resident scan.
 * k = 1 is vgicp_align_resident.
 *
 * A hypothesis whose solved pose is not finite gets VGICP_ERR_DEGENERATE in status[h], and its pose is written as the
 * single call writes it; the call itself returns VGICP_OK and the other hypotheses are unaffected.  With status ==
 * NULL (or stats == NULL) the call returns the first hypothesis status that is not VGICP_OK.  Any other error ends the
 * call at once and is returned.
 *
 * The scan generation counter does not move and the map is not touched.  A scan that is still pending (after
 * vgicp_scan_prepare_async) is settled FIRST — one extra host synchronisation, which vgicp_align_resident does not
 * need: the team layout is made from the kept count, not from the raw count.  A pending map insertion is settled as
 * vgicp_align_resident settles it (here: in that same synchronisation).
 *
 * Nothing is allocated inside the call, on the device or page-locked: the batch's exchange words (576 KB on the
 * device), its state and log (VGICP_BATCH_MAX hypotheses x 64 rounds, 1 MB page-locked) are made by vgicp_create.  The
 * exchange words of vgicp_align_resident and their rotation are not touched by a batch.
 *
 * Every wait is bounded.  If a workgroup of a batch launch gives up waiting, the whole batch is run again as k single
 * aligns with one launch per iteration: VGICP_COUNTER_PERSISTENT_FALLBACKS goes up by ONE, the next 8 aligns (a batch
 * counts as k) use one launch per iteration as well, and the results are the same bits.
 *
 * These run the k aligns one after another through vgicp_align_resident's own paths — the same results,
 * hypotheses_per_launch = 1: multi-device contexts, communicators and peer-connected contexts, VGICP_FLAG_NO_PERSISTENT,
 * VGICP_FLAG_PROFILE (kernel_ms is not reported), VGICP_DEBUG_STAMPS, max_iteration = 0 or > 63, scans of more than
 * grid x 448 points (several points per thread; grid = min(compute units, 256)) and scans too large for two teams
 * (more than floor(grid / 2) x 448 points). */
int vgicp_align_resident_batch(vgicp_ctx* ctx, size_t k, const double* guesses /* k x 16 */,
                               const vgicp_params* params, double* out_poses /* k x 16 */,
                               vgicp_batch_stats* stats);

/* How many hypotheses one launch takes for the scan that is resident now: min(16, floor(grid / ceil(n / 448))), or 1
 * where a batch would run its aligns one after another whatever the flags (see above).  Settles a pending scan.
 * VGICP_ERR_NOT_READY without a resident scan. */
int vgicp_align_batch_width(vgicp_ctx* ctx, size_t* hypotheses_per_launch);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_BATCH_H_ */
