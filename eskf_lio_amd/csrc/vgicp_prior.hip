// vgicp_prior.hip — libvgicp_hip_prior.so: the two entry points of include/vgicp_hip_prior.h.
// The pose prior: the checks of vgicp_set_pose_prior, what the context keeps of it, and the chart on the host.  No GPU
// call and no kernel: the prior reaches the kernels of libvgicp_hip.so in the launch arguments (prior_args,
// vgicp_context.h).  A library of its own because libvgicp_hip.so's exported vgicp_* names are pinned to the lists of
// the headers before this one; it writes three fields of vgicp_ctx and the error text, so it is built from the same
// vgicp_context.h as the module beside it (one Makefile, one rule set) and links against it.
#include <algorithm>
#include <cmath>

#include "vgicp_context.h"

namespace {
// Is the symmetric 6x6 (lower triangle of the column-major L) positive semi-definite?  LDL^T with diagonal pivoting:
// every pivot >= -tol; once the largest remaining diagonal entry is within tol of zero, what remains must be zero to tol.
bool prior_info_is_psd(const double* L, double tol) {
  double A[6][6];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) A[r][c] = r >= c ? L[r + 6 * c] : L[c + 6 * r];
  for (int k = 0; k < 6; ++k) {
    int p = k;
    for (int i = k + 1; i < 6; ++i)
      if (A[i][i] > A[p][p]) p = i;
    for (int i = k; i < 6; ++i)
      if (A[i][i] < -tol) return false;
    if (A[p][p] <= tol) {
      for (int r = k; r < 6; ++r)
        for (int c = k; c < 6; ++c)
          if (std::fabs(A[r][c]) > tol) return false;
      return true;
    }
    if (p != k) {
      for (int c = 0; c < 6; ++c) std::swap(A[k][c], A[p][c]);
      for (int r = 0; r < 6; ++r) std::swap(A[r][k], A[r][p]);
    }
    for (int r = k + 1; r < 6; ++r)
      for (int c = k + 1; c < 6; ++c) A[r][c] -= A[r][k] * A[k][c] / A[k][k];
  }
  return true;
}
}  // namespace

extern "C" {

int vgicp_set_pose_prior(vgicp_ctx* ctx, const double prior_pose[16], const double information[36]) {
  VG_RC(layout_handshake(ctx, "libvgicp_hip_prior.so and the libvgicp_hip.so that created this context are not from one build"));
  if (!prior_pose || !information) {   // a clear: never refused, and vgicp_last_error keeps its text
    ctx->prior_on = false;
    return VGICP_OK;
  }
  if (ctx->multi)
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the pose prior (vgicp_hip_prior.h) runs on a single-device context only");
  double biggest = 0.0;
  for (int k = 0; k < 36; ++k) {
    if (!std::isfinite(information[k])) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the prior's information has an entry that is not finite");
    biggest = std::max(biggest, std::fabs(information[k]));
  }
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(prior_pose[k])) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the prior pose has an entry that is not finite");
  const double tol = 1e-12 * biggest;
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < r; ++c)
      if (std::fabs(information[r + 6 * c] - information[c + 6 * r]) > tol)
        return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the prior's information is not symmetric");
  if (!prior_info_is_psd(information, tol))
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the prior's information is not positive semi-definite");
  if (prior_pose[3] != 0.0 || prior_pose[7] != 0.0 || prior_pose[11] != 0.0 || prior_pose[15] != 1.0)
    return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the prior pose's last row is not 0 0 0 1");
  Pose T0;
  pose_from_mat4(prior_pose, T0);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b <= a; ++b) {
      const double dot = T0.R[3 * a] * T0.R[3 * b] + T0.R[3 * a + 1] * T0.R[3 * b + 1] + T0.R[3 * a + 2] * T0.R[3 * b + 2];
      if (std::fabs(dot - (a == b ? 1.0 : 0.0)) > 1e-9)
        return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the prior pose's rotation block is not orthonormal");
    }
  // a reflection passes the column test: det = +1 is part of "rotation"
  const double det = T0.R[0] * (T0.R[4] * T0.R[8] - T0.R[7] * T0.R[5]) - T0.R[3] * (T0.R[1] * T0.R[8] - T0.R[7] * T0.R[2]) +
                     T0.R[6] * (T0.R[1] * T0.R[5] - T0.R[4] * T0.R[2]);
  if (det < 0.0) return fail(ctx, VGICP_ERR_BAD_ARGUMENT, "the prior pose's rotation block is a reflection");
  if (biggest == 0.0) {   // no information: no prior
    ctx->prior_on = false;
    return VGICP_OK;
  }
  ctx->prior_on = true;
  for (int k = 0; k < 9; ++k) ctx->prior_pose[k] = T0.R[k];
  for (int k = 0; k < 3; ++k) ctx->prior_pose[9 + k] = T0.t[k];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c <= r; ++c) ctx->prior_info[tri6(r, c)] = information[r + 6 * c];
  return VGICP_OK;
}

int vgicp_pose_prior_chart(const double prior_pose[16], const double pose[16], double d[6], double G[36]) {
  if (!prior_pose || !pose) return VGICP_ERR_BAD_ARGUMENT;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(prior_pose[k]) || !std::isfinite(pose[k])) return VGICP_ERR_BAD_ARGUMENT;
  Pose T0, T;
  pose_from_mat4(prior_pose, T0);
  pose_from_mat4(pose, T);
  double dd[6], GG[36];
  pose_prior_chart(T0, T, dd, GG);
  if (d) for (int k = 0; k < 6; ++k) d[k] = dd[k];
  if (G) for (int k = 0; k < 36; ++k) G[k] = GG[k];
  return VGICP_OK;
}
}  // extern "C"
