/* vgicp_hip_robust.h — extension of the C ABI (vgicp_hip.h): robust rounds.
 *
 * The reference's registration is plain least squares: a point whose voxel exists in the map enters the normal
 * equations with full weight, however far it lies from that voxel's distribution (src/Registration.cpp:44-72).  The three
 * options below give every round of an align a correspondence GATE on the squared Mahalanobis residual and a robust
 * WEIGHT (Huber or Cauchy), as users of a GICP library expect.  This header declares no function: the main header's list
 * of entry points is pinned, VGICP_ABI_VERSION stays 6, vgicp_params and vgicp_stats keep their layout.  The mode is
 * set with vgicp_set_option, holds per context until it is changed, and with all three options at their defaults the
 * plain path runs, bit for bit.
 *
 * What a round computes while the mode is on:
 *   - A correspondence is what it is without the mode: the exact-voxel lookup, unchanged.
 *   - e = R p + t - mu_voxel, W = (R C R^T + C_voxel)^-1 as the plain round forms them; d^2 = max(e^T W e, 0).
 *   - Gate g > 0: a correspondence with !(e^T W e <= g) has weight 0 and is NOT counted (a NaN residual is rejected).
 *     A rejected correspondence adds +0 to every sum of the round, whatever its covariances hold: a scan point whose
 *     covariance has a non-finite entry leaves a gated round's sums finite.
 *   - Huber, scale c:   w = 1 if d^2 <= c^2, else c / sqrt(d^2).
 *   - Cauchy, scale c:  w = 1 / (1 + d^2 / c^2).
 *   - The round solves (sum w J^T W J) xi = - sum w J^T W e.  The weights come from the pose the round starts with:
 *     plain iteratively reweighted least squares (IRLS).  Solve, exponential, compose and the convergence test are
 *     untouched.
 *   - vgicp_stats.corr_count[r] counts the correspondences of round r with a non-zero weight, vgicp_stats.normal_eq[r]
 *     is the WEIGHTED system.  A round in which the gate rejects everything behaves as a round without any match.
 *
 * UNITS.  The map's and the scan's covariances are the reference's REGULARISED ones (eigenvalues normalised to
 * 1, 1, 1e-2), so d^2 is not a chi-square value: sensible scales and gates are around 0.1, not around 3.  On the
 * synthetic scene of tests/test_robust.py at the true pose, d^2 of the points that belong to the map has median 0.0023
 * and 99th percentile 0.032; points displaced by 9 cm have median 0.088.  To pick values for real data, score a pose
 * with vgicp_evaluate_resident, declared in vgicp_hip_evaluate.h: cost / correspondences is the mean d^2 at that pose.
 * For the distribution itself, vgicp_points_resident, declared in vgicp_hip_points.h, returns d^2 and the weight of every
 * point of the resident scan at a pose, and order statistics of d^2 (a median, a 99th percentile) to set c and g by.
 *
 * SCOPE.  The mode applies to vgicp_align, vgicp_align_resident and vgicp_align_resident_batch on a single-device
 * context.  While it is on
 *   - vgicp_align uploads the scan and then aligns it as vgicp_align_resident does (no fused upload launch);
 *   - vgicp_align_resident_batch runs its k hypotheses one by one (hypotheses_per_launch = 1, vgicp_align_batch_width
 *     reports 1): each is the single call, bit for bit;
 *   - vgicp_accumulate, vgicp_match and vgicp_evaluate_resident stay UNWEIGHTED: scores are the plain objective;
 *   - a context with a communicator (vgicp_comm_init) or connected peers (vgicp_peer_connect) refuses the align with
 *     VGICP_ERR_BAD_ARGUMENT and a text in vgicp_last_error;
 *   - a multi-device context (vgicp_create_multi) refuses the three options themselves, with a text.
 * Several devices are out of scope: the rows the devices exchange would carry the weighted sums unchanged, but that path
 * has not been tested.
 *
 * A value that is refused (VGICP_ERR_BAD_ARGUMENT) changes nothing. */
#ifndef VGICP_HIP_ROBUST_H_
#define VGICP_HIP_ROBUST_H_

#include "vgicp_hip.h"

/* Options of vgicp_set_option. */
#define VGICP_OPTION_ROBUST_KERNEL 5      /* VGICP_ROBUST_NONE (default), _HUBER or _CAUCHY; anything else is refused */
#define VGICP_OPTION_ROBUST_SCALE_MICRO 6 /* c = (double)value / 1000000.0, value >= 1; default 1000000 (c = 1) */
#define VGICP_OPTION_GATE_MICRO 7         /* gate on d^2 = (double)value / 1000000.0; 0 = no gate (default); < 0 refused */

/* Values of VGICP_OPTION_ROBUST_KERNEL. */
#define VGICP_ROBUST_NONE 0
#define VGICP_ROBUST_HUBER 1
#define VGICP_ROBUST_CAUCHY 2

#endif /* VGICP_HIP_ROBUST_H_ */
