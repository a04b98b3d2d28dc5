"""The reference of the robust-round tests (include/vgicp_hip_robust.h): iteratively reweighted least squares built from
the CPU oracle's pieces, and the scene both test files use.  Not a test module.

One round, from the oracle's own state (the cloud moved by every step so far, as oracle_align moves it):
  correspondences  OracleMap.match
  per-term blocks  oracle.jtj_jtr (ICP::computeJTJAndJTr), cov = source + map covariance
  d^2              max(e^T (C_src + C_map)^-1 e, 0) by Cramer's rule in extended precision, as reference_sums of
                   tests/test_evaluate.py forms its cost terms (copied from there)
  weights          the header's formulas, in fp64 from that d^2
  sums             numpy, in point order: with every weight 1.0 the products are exact and the sums are the oracle's own
  tail             oracle.solve_step, the oracle's compose restated, oracle.convergence_check
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

DISPLACEMENT = (0.06, -0.05, 0.04)     # metres, map frame: every fifth point of the scene's scan
MAX_IT, TSQ, COS = 30, 1e-12, 1.0 - 1e-12
NONE, HUBER, CAUCHY = 0, 1, 2
# the modes of the issue's table: name -> (kernel, scale c, gate on d^2)
MODES = {
    "cauchy": (CAUCHY, 0.15, 0.0),
    "huber": (HUBER, 0.08, 0.0),
    "gate": (NONE, 1.0, 0.04),
    "cauchy+gate": (CAUCHY, 0.10, 0.06),
}


def make_scene(n=6000, voxels=20_000):
    """(vmap, points, covariances, T_true, guess): a structured scan of the map, every fifth point displaced by
    DISPLACEMENT in the map frame, so that it stays in or next to its voxel."""
    from eskf_lio_amd import synth
    vmap = synth.make_map(voxels)
    pts, covs, T_true = synth.make_structured_scan(n, vmap)
    pts = pts.copy()
    pts[::5] += T_true[:3, :3].T @ np.array(DISPLACEMENT)    # p_map + d = R (p + R^T d) + t
    return vmap, pts, covs, T_true, synth.default_guess()


def mahalanobis_sq(sp, sc, mp, mc):
    """e^T (sc + mc)^-1 e per correspondence in extended precision (64-bit significand), rounded once to fp64."""
    m = sp.shape[0]
    S = sc.astype(np.longdouble).reshape(m, 3, 3) + mc.astype(np.longdouble).reshape(m, 3, 3)
    e = sp.astype(np.longdouble) - mp.astype(np.longdouble)
    det = (S[:, 0, 0] * (S[:, 1, 1] * S[:, 2, 2] - S[:, 1, 2] * S[:, 2, 1])
           - S[:, 0, 1] * (S[:, 1, 0] * S[:, 2, 2] - S[:, 1, 2] * S[:, 2, 0])
           + S[:, 0, 2] * (S[:, 1, 0] * S[:, 2, 1] - S[:, 1, 1] * S[:, 2, 0]))
    adj = np.empty_like(S)
    for r in range(3):
        for c in range(3):
            r0, r1 = [k for k in range(3) if k != c]      # adj[r][c] = cofactor[c][r]
            c0, c1 = [k for k in range(3) if k != r]
            adj[:, r, c] = (-1) ** (r + c) * (S[:, r0, c0] * S[:, r1, c1] - S[:, r0, c1] * S[:, r1, c0])
    x = np.einsum("mrc,mc->mr", adj, e) / det[:, None]
    return np.einsum("mr,mr->m", e, x).astype(np.float64)


def weights(d2_raw, kernel, c, gate):
    """The header's formulas: (weight per correspondence, d^2).  gate 0 = none; a NaN residual fails the gate."""
    d2 = np.maximum(d2_raw, 0.0)
    if kernel == HUBER:
        with np.errstate(divide="ignore"):
            w = np.where(d2 <= c * c, 1.0, c / np.sqrt(d2))
    elif kernel == CAUCHY:
        w = 1.0 / (1.0 + d2 / (c * c))
    else:
        w = np.ones_like(d2)
    if gate > 0.0:
        w = np.where(d2_raw <= gate, w, 0.0)
    return w, d2


def term_blocks(oracle, sp, mp, S):
    """oracle.jtj_jtr for every correspondence: (m x 36 column-major, m x 6), without a numpy allocation per call."""
    lib = oracle.load()
    m = sp.shape[0]
    sp, mp, S = np.ascontiguousarray(sp), np.ascontiguousarray(mp), np.ascontiguousarray(S)
    H, b = np.zeros((m, 36)), np.zeros((m, 6))
    dp = C.POINTER(C.c_double)
    a_sp, a_mp, a_S, a_H, a_b = (x.ctypes.data for x in (sp, mp, S, H, b))
    fn = lib.oracle_jtj_jtr
    for i in range(m):
        fn(C.cast(a_sp + 24 * i, dp), C.cast(a_mp + 24 * i, dp), C.cast(a_S + 72 * i, dp), C.cast(a_H + 288 * i, dp),
           C.cast(a_b + 48 * i, dp))
    return H, b


def compose(A, B):
    """The oracle's Isometry3d * Isometry3d (oracle/vgicp_oracle.cpp: compose), operation for operation."""
    out = np.eye(4)
    for c in range(4):
        for r in range(3):
            s = float(A[r, 0]) * float(B[0, c])
            s += float(A[r, 1]) * float(B[1, c])
            s += float(A[r, 2]) * float(B[2, c])
            if c == 3:
                s += float(A[r, 3])
            out[r, c] = s
    return out


def packed(JTJ, JTr):
    """6 x 6 and 6 -> the 27 doubles of vgicp_stats.normal_eq: lower triangle row by row, then J^T r."""
    return np.array([JTJ[r, c] for r in range(6) for c in range(r + 1)] + list(JTr))


@dataclass
class RobustAlign:
    pose: np.ndarray
    iterations: int
    converged: bool
    corr_count: np.ndarray      # correspondences with a non-zero weight, per round
    matched: np.ndarray         # correspondences before the gate, per round
    normal_eq: np.ndarray       # rounds x 27, the weighted system
    d2: list                    # per round: the raw residuals e^T W e of the matched points
    gate_margin: float          # smallest |d^2 - gate| / gate over all rounds (inf without a gate)


def irls_align(oracle, om, pts, covs, guess, kernel=NONE, c=1.0, gate=0.0, max_it=MAX_IT, tsq=TSQ, cos=COS):
    total = np.array(guess, dtype=np.float64)
    tp, tc = oracle.transform(pts, covs, total)
    counts, matched, rows, d2s = [], [], [], []
    margin, converged = float("inf"), False
    for _ in range(max_it):
        sp, sc, mp, mc, _ = om.match(tp, tc)
        m = sp.shape[0]
        JTJ, JTr = np.zeros((6, 6)), np.zeros(6)
        raw = np.zeros(0)
        kept = 0
        if m:
            H, b = term_blocks(oracle, sp, mp, sc + mc)
            raw = mahalanobis_sq(sp, sc, mp, mc)
            w, _ = weights(raw, kernel, c, gate)
            if gate > 0.0:
                margin = min(margin, float(np.abs(raw - gate).min() / gate))
            kept = int(np.count_nonzero(w > 0.0))
            # in point order, as the oracle's deterministic pass adds them
            JTJ = np.cumsum(H * w[:, None], axis=0)[-1].reshape(6, 6).T.copy()
            JTr = np.cumsum(b * w[:, None], axis=0)[-1]
        counts.append(kept)
        matched.append(m)
        rows.append(packed(JTJ, JTr))
        d2s.append(raw)
        _, step = oracle.solve_step(JTJ, JTr)
        total = compose(step, total)
        if oracle.convergence_check(step, cos, tsq):
            converged = True
            break
        tp, tc = oracle.transform(tp, tc, step)
    return RobustAlign(total, len(counts), converged, np.array(counts, dtype=np.uint64), np.array(matched, dtype=np.uint64),
                       np.array(rows).reshape(len(rows), 27), d2s, margin)


def translation_error(pose, T_true):
    return float(np.linalg.norm(pose[:3, 3] - T_true[:3, 3]))
