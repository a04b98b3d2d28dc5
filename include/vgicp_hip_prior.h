/* vgicp_hip_prior.h — extension of the C ABI (vgicp_hip.h): align with a Gaussian prior on the pose.
 *
 * The reference couples LiDAR and IMU loosely: ErrorStateKF::update (src/ErrorStateKF.cpp:115-162) hands ICP::align the
 * mean of its state as the guess and nothing of its covariance, so a round whose 6x6 is badly conditioned (a corridor, an
 * open field, few correspondences) is solved from the data alone.  With a prior set, the pose block of the filter's
 * information enters the normal equations of EVERY round, and the pose an align returns is the MAP estimate (an
 * iterated Kalman update) — what users of small_gicp and fast_gicp know as a prior factor.
 *
 * Declared here and not in vgicp_hip.h: the main header's list of entry points is pinned, and so is the set of names
 * libvgicp_hip.so exports.  Both functions are defined in libvgicp_hip_prior.so, built beside libvgicp_hip.so from the
 * same sources and to be linked with it (-lvgicp_hip -lvgicp_hip_prior); the kernels of the prior's rounds are in
 * libvgicp_hip.so itself.  VGICP_ABI_VERSION is unchanged, vgicp_params and vgicp_stats keep their layout.
 * With no prior set every path runs as it does without this header, bit for bit.
 *
 * THE MATHEMATICS.  A prior is a pose T0 = (R0, t0) and a symmetric positive semi-definite 6x6 information matrix L,
 * expressed in the ESKF's own chart, the residual of src/ErrorStateKF.cpp:132-135:
 *
 *     d(T) = [ t - t0 ;  Log(R0^T R) ]            (translation first, then the rotation vector)
 *
 * An align minimises  sum e_i^T W_i e_i + d(T)^T L d(T).  The data terms carry no factor 1/2 in the reference's normal
 * equations, so L is added as it is.  A round's increment is the reference's xi = (v, omega) with T <- se3ToSE3(xi) T;
 * at the round's pose (R, t) the chart's Jacobian with respect to xi is
 *
 *     G = [ I    -[t]x          ]        phi = Log(R0^T R),  theta = |phi|
 *         [ 0    Jr^-1(phi) R^T ]
 *     Jr^-1(phi) = I + 1/2 [phi]x + c(theta) [phi]x^2,   c(theta) = 1/theta^2 - (1 + cos theta) / (2 theta sin theta)
 *
 * (c by its power series, limit 1/12, for theta^2 <= 0.25 — where the kernels' se(3) exponential leaves its own series),
 * and the round solves
 *
 *     (A + G^T L G) xi = -(b + G^T L d)
 *
 * where A and b are the folded data sums the round has without a prior.  Exponential, compose and the convergence test
 * are untouched.  A round without a single match still solves with the prior's terms, so the pose walks to T0.
 *
 * vgicp_stats.corr_count[r] and vgicp_stats.normal_eq[r] stay the DATA sums of round r (the weighted ones with the robust
 * mode on): the prior is added only in front of the solve, so vgicp_evaluate_resident's information and every consumer
 * of the log mean what they mean without a prior.  Round 0's row therefore equals the plain align's from the same guess.
 *
 * SCOPE: exactly the robust mode's (vgicp_hip_robust.h), for the same reason — the prior's round has instantiations of
 * the single-device persistent launch and of the launch-per-round loop only.  While a prior is set
 *   - vgicp_align_resident takes the persistent launch or the loop, as the plan decides without a prior;
 *   - vgicp_align uploads the scan and then aligns it as vgicp_align_resident does (no fused upload launch);
 *   - vgicp_align_resident_batch runs its k hypotheses one by one (hypotheses_per_launch = 1, vgicp_align_batch_width
 *     reports 1): each is the single call, bit for bit — one prior from the filter, a fan of starting points;
 *   - vgicp_accumulate, vgicp_match, vgicp_solve_step and vgicp_evaluate_resident ignore the prior;
 *   - a context with a communicator (vgicp_comm_init) or connected peers (vgicp_peer_connect) refuses the align with
 *     VGICP_ERR_BAD_ARGUMENT and a text in vgicp_last_error;
 *   - a multi-device context (vgicp_create_multi) refuses vgicp_set_pose_prior itself, with a text.
 * The prior and the robust mode combine: the weighted sums are A and b, the prior is added on top. */
#ifndef VGICP_HIP_PRIOR_H_
#define VGICP_HIP_PRIOR_H_

#include "vgicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sets the prior of every later align of this context.  prior_pose: laid out as vgicp_align_resident's guess.
 * information: column-major 6x6, only the lower triangle is read after the symmetry check.  NULL pose or NULL
 * information, or an information that is all zero: the prior is cleared.  Sticky until cleared or replaced.
 *
 * Refused with VGICP_ERR_BAD_ARGUMENT, a text in vgicp_last_error and nothing changed:
 *   - an entry that is not finite;
 *   - |L_ij - L_ji| above 1e-12 max|L|;
 *   - an L that is not positive semi-definite (a host-side pivoted LDL^T: every pivot >= -1e-12 max|L|);
 *   - a prior_pose whose rotation block is not orthonormal to 1e-9 or is a reflection (determinant < 0), or whose
 *     last row is not 0 0 0 1;
 *   - a multi-device context;
 *   - a context created by a libvgicp_hip.so of another build than this libvgicp_hip_prior.so (the pair shares the
 *     context's layout and must come from one build; the context is then neither read nor written, and the text is at
 *     vgicp_last_error(NULL)).
 * A clear is never refused and leaves vgicp_last_error's text alone. */
int vgicp_set_pose_prior(vgicp_ctx* ctx, const double prior_pose[16], const double information[36]);

/* Host only, no context, no GPU: d (6) and G (36, column-major) of the chart above for `pose` against `prior_pose`,
 * with the very formulas the kernels use (one source, vgicp_math.h) — so that a caller can carry an information matrix
 * between the xi chart of normal_eq and the filter's chart.  Either output may be NULL.  VGICP_ERR_BAD_ARGUMENT for a
 * NULL or non-finite input. */
int vgicp_pose_prior_chart(const double prior_pose[16], const double pose[16], double d[6], double G[36]);

#ifdef __cplusplus
}
#endif

#endif /* VGICP_HIP_PRIOR_H_ */
