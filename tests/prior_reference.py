"""The reference of the pose-prior tests (include/vgicp_hip_prior.h): Gauss-Newton with a Gaussian prior on the pose,
built from the CPU oracle's pieces and a numpy restatement of the header's chart.  Not a test module.

One round, from the oracle's own state (the cloud moved by every step so far, as oracle_align moves it):
  correspondences  OracleMap.match
  data sums        oracle.jtj_jtr per term, with robust_reference's weights when a robust mode is on, numpy sums in point
                   order (robust_reference.irls_align's round)
  prior            d, G and Jr^-1 below, written out from the header's equations — NOT through vgicp_pose_prior_chart
  solve            numpy.linalg.solve on the dense symmetric (A + G^T L G) xi = -(b + G^T L d)
  tail             oracle.se3_to_SE3, the oracle's compose restated, oracle.convergence_check
"""
from dataclasses import dataclass

import numpy as np

import robust_reference as rr

SERIES_MAX2 = 0.25      # theta^2 up to which c(theta) takes its series: where se3_exp_device leaves its own (n2 > 0.25)
# |B_2k| / (2k)!, k = 1 .. 8: c(theta) = sum_k coefficient_k theta^(2k - 2)
C_SERIES = (1 / 12, 1 / 720, 1 / 30240, 1 / 1209600, 1 / 47900160, 691 / 1307674368000, 1 / 74724249600,
            3617 / 10670622842880000)


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_exp(phi):
    """Rodrigues, for building test poses."""
    phi = np.asarray(phi, dtype=np.float64)
    th = float(np.linalg.norm(phi))
    K = hat(phi)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * K @ K


def so3_log(M):
    """Rotation vector of a rotation matrix, |phi| <= pi."""
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    s, c = float(np.linalg.norm(v)), 0.5 * (np.trace(M) - 1.0)
    th = float(np.arctan2(s, c))
    if c > -0.9:
        return v * (th / s) if s > 1e-150 else v.copy()
    # near pi: the axis is the eigenvector of the symmetric part for its largest eigenvalue, signed by v
    w, V = np.linalg.eigh(0.5 * (M + M.T))
    a = V[:, -1]
    if np.dot(a, v) < 0.0:
        a = -a
    return th * a


def c_theta(th):
    """c(theta) of Jr^-1: the closed form of the header, its series for theta^2 <= SERIES_MAX2 (limit 1/12)."""
    n2 = th * th
    if n2 > SERIES_MAX2:
        return 1.0 / n2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return float(sum(ck * n2 ** k for k, ck in enumerate(C_SERIES)))


def jr_inv(phi):
    K = hat(phi)
    return np.eye(3) + 0.5 * K + c_theta(float(np.linalg.norm(phi))) * K @ K


def chart(T0, T):
    """(d (6), G (6 x 6)) of the header: d = [t - t0; Log(R0^T R)], G = [I, -[t]x; 0, Jr^-1(phi) R^T]."""
    R0, t0, R, t = T0[:3, :3], T0[:3, 3], T[:3, :3], T[:3, 3]
    phi = so3_log(R0.T @ R)
    d = np.concatenate([t - t0, phi])
    G = np.zeros((6, 6))
    G[:3, :3] = np.eye(3)
    G[:3, 3:] = -hat(t)
    G[3:, 3:] = jr_inv(phi) @ R.T
    return d, G


@dataclass
class PriorAlign:
    pose: np.ndarray
    iterations: int
    converged: bool
    corr_count: np.ndarray      # correspondences with a non-zero weight, per round
    normal_eq: np.ndarray       # rounds x 27: the DATA sums (weighted with a robust mode), without the prior


def prior_align(oracle, om, pts, covs, guess, T0, L, kernel=rr.NONE, c=1.0, gate=0.0, max_it=rr.MAX_IT, tsq=rr.TSQ,
                cos=rr.COS):
    total = np.array(guess, dtype=np.float64)
    T0, L = np.asarray(T0, dtype=np.float64), np.asarray(L, dtype=np.float64)
    tp, tc = oracle.transform(pts, covs, total)
    counts, rows, converged = [], [], False
    for _ in range(max_it):
        sp, sc, mp, mc, _ = om.match(tp, tc)
        m = sp.shape[0]
        JTJ, JTr, kept = np.zeros((6, 6)), np.zeros(6), 0
        if m:
            H, b = rr.term_blocks(oracle, sp, mp, sc + mc)
            w = np.ones(m)
            if kernel != rr.NONE or gate > 0.0:
                w, _ = rr.weights(rr.mahalanobis_sq(sp, sc, mp, mc), kernel, c, gate)
            kept = int(np.count_nonzero(w > 0.0))
            JTJ = np.cumsum(H * w[:, None], axis=0)[-1].reshape(6, 6).T.copy()
            JTr = np.cumsum(b * w[:, None], axis=0)[-1]
        counts.append(kept)
        rows.append(rr.packed(JTJ, JTr))
        d, G = chart(T0, total)
        A = JTJ + G.T @ L @ G
        xi = np.linalg.solve(0.5 * (A + A.T), -(JTr + G.T @ (L @ d)))
        step = oracle.se3_to_SE3(xi)
        total = rr.compose(step, total)
        if oracle.convergence_check(step, cos, tsq):
            converged = True
            break
        tp, tc = oracle.transform(tp, tc, step)
    return PriorAlign(total, len(counts), converged, np.array(counts, dtype=np.uint64),
                      np.array(rows).reshape(len(rows), 27))
