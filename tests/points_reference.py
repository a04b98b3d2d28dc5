"""The reference of the per-point tests (include/vgicp_hip_points.h): what vgicp_points_resident reports, formed from the
CPU oracle's transform and match and from tests/robust_reference.py (d^2 in extended precision, the header's weights).
Not a test module; tests/test_points_cpu.py checks the preconditions on it alone, tests/test_points.py holds the device
against it."""
import math
from dataclasses import dataclass

import numpy as np

import robust_reference as rr

U = 2.0 ** -53                       # unit roundoff of fp64
COST_C = 72                          # first-order operation count of one cost term: COST_C of tests/test_evaluate.py
GATES = (0.01, 0.02, 0.04, 0.06, 0.1)
QS = (0.0, 0.25, 0.5, 0.9, 0.99, 1.0)
MATCHED, NEGATIVE, NOT_FINITE = 1, 2, 4


@dataclass
class PointsRef:
    n: int
    index: np.ndarray      # indices of the matched points, ascending
    raw: np.ndarray        # e^T W e of the matched points (may be negative or NaN)
    sq: np.ndarray         # |e|^2 of the matched points
    kappa: float           # largest 2-norm condition number of S = src_cov + map_cov over the finite matched pairs

    def prefix(self, n):
        keep = self.index < n
        return PointsRef(n, self.index[keep], self.raw[keep], self.sq[keep], self.kappa)

    @property
    def ranked(self):
        """max(raw, 0) of the matched points with a finite raw, ascending."""
        return np.sort(np.maximum(self.raw[np.isfinite(self.raw)], 0.0))

    def planes(self, kernel=rr.NONE, c=1.0, gate=0.0):
        """(d2, sq_error, weight, status) over all n points, as the header defines them."""
        d2, sq, w = np.full(self.n, np.inf), np.full(self.n, np.inf), np.zeros(self.n)
        status = np.zeros(self.n, dtype=np.uint8)
        d2[self.index], sq[self.index] = self.raw, self.sq
        with np.errstate(invalid="ignore"):
            w[self.index] = rr.weights(self.raw, kernel, c, gate)[0]
            bad = ~np.isfinite(self.raw)
            status[self.index] = MATCHED + NOT_FINITE * bad + NEGATIVE * (~bad & (self.raw < 0.0))
        return d2, sq, w, status


def reference_at(oracle, om, pts, covs, pose):
    tp, tc = oracle.transform(pts, covs, pose)
    sp, sc, mp, mc, ix = om.match(tp, tc)
    m = sp.shape[0]
    if m == 0:
        return PointsRef(pts.shape[0], np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0), 1.0)
    with np.errstate(invalid="ignore"):
        raw = rr.mahalanobis_sq(sp, sc, mp, mc)
    e = sp.astype(np.longdouble) - mp.astype(np.longdouble)
    sq = np.einsum("mr,mr->m", e, e).astype(np.float64)
    S = (sc + mc).reshape(m, 3, 3)
    fine = np.isfinite(S).all(axis=(1, 2))
    kappa = float(np.linalg.cond(S[fine]).max()) if fine.any() else 1.0
    order = np.argsort(ix, kind="stable")
    return PointsRef(pts.shape[0], np.asarray(ix, dtype=np.int64)[order], raw[order], sq[order], kappa)


def quantile_rank(q, m):
    """The header's rank in Python integers: min(max(ceil(q m), 1), m) - 1; the product is fp64's."""
    return min(max(math.ceil(q * m), 1), m) - 1


def order_statistics(sorted_values, qs):
    m = len(sorted_values)
    return np.array([sorted_values[quantile_rank(q, m)] if m else np.nan for q in qs])


def smallest_relative_gap(sorted_values):
    v = sorted_values[sorted_values > 0.0]
    return float(((v[1:] - v[:-1]) / v[1:]).min())


def gate_margin(raw, gate):
    return float(np.abs(raw - gate).min() / gate)
