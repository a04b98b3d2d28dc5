"""The solver-domain tests' own ground, without a device: tests/solver_reference.py (extended precision) against the two
references the suite already trusts and against 50-digit arithmetic, and the proof that the device test of the
exponential (tests/test_solver_domain.py) would notice a wrong digit in se3_exp_device's series."""
import numpy as np
import pytest

import prior_reference as pr
import solver_reference as sr

pytestmark = pytest.mark.skipif(sr.unavailable_reason() is not None, reason=str(sr.unavailable_reason()))

EPS = sr.EPS
LD = sr.LD


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- the reference against the existing references ---------------------------------------------------------------------
def test_exponential_equals_the_oracles(oracle):
    """sr.se3_exp against oracle.se3_to_SE3 (angle-axis in fp64, J_l = I below 1e-6 rad) over the whole range of the
    device test.  The oracle's own error: the angle is rounded (eps |phi| into every entry), the axis is normalised by a
    division, and each entry is two or three products and sums — 16 eps max(1, |rho|_inf) (1 + |phi|), four times the
    bound the device has to meet, covers it.  On top of that the oracle's J_l (the reference implementation's formula)
    forms f2 = (1 - cos a) / a from a cosine that is rounded to eps / 2 next to 1: an absolute eps / (2 a) in f2, which
    multiplies k x rho, |k x rho| <= sqrt(3) |rho|_inf — eps |rho|_inf / a, 1e-10 |rho|_inf just above the 1e-6 switch.
    (The device's series has no such term; that is why this comparison cannot stand in for the device test.)
    Observed: 0.34 of the tolerance at worst."""
    worst = 0.0
    for name, rho, phi, small in sr.exp_sweep():
        R, t = sr.se3_exp_many(rho, phi, small)
        angle = np.maximum(np.linalg.norm(phi, axis=1), 1e-300)
        tol = 4.0 * sr.exp_bound(rho, phi) + np.where(small, 0.0, EPS * np.abs(rho).max(axis=1) / angle)
        for k in range(0, len(phi), 3):                      # every third input: 1 600 oracle calls
            T = oracle.se3_to_SE3(np.r_[rho[k], phi[k]])
            diff = max(np.abs(f64(R[k] - T[:3, :3].astype(LD))).max(), np.abs(f64(t[k] - T[:3, 3].astype(LD))).max())
            worst = max(worst, diff / tol[k])
            assert diff <= tol[k], (name, rho[k], phi[k], diff, tol[k])
    print(f"worst |sr - oracle| / tolerance {worst:.3f}")


@pytest.mark.parametrize("theta", (0.0, 1e-9, 1e-6, 1e-3, 0.09, 0.11, 0.5, 1.0, np.pi / 2, 2.5, 3.1))
def test_chart_equals_prior_references(theta):
    """sr.chart (Log by so3_log of the fp64 matrices, and with phi given by construction) against prior_reference.chart,
    to the accuracy tests/test_prior_cpu.py states for the latter: 64 eps x 24 x S, S = 1 + |t| + theta."""
    rng = np.random.default_rng(int(theta * 1000) + 3)
    for _ in range(20):
        axis = sr.unit_axes(rng, 1)[0]
        T0, T = np.eye(4), np.eye(4)
        T0[:3, :3] = pr.so3_exp(rng.uniform(-2.0, 2.0, size=3))
        T0[:3, 3], T[:3, 3] = rng.normal(size=3) * 3.0, rng.normal(size=3) * 3.0
        T[:3, :3] = f64(T0[:3, :3].astype(LD) @ sr.so3_exp(theta, axis))
        d_ref, G_ref = pr.chart(T0, T)
        tol = 64 * EPS * 24 * (1.0 + np.linalg.norm(T[:3, 3]) + theta)
        for phi in (None, LD(theta) * axis.astype(LD)):
            d, G = sr.chart(T0, T, phi)
            assert np.abs(f64(d) - d_ref).max() <= tol and np.abs(f64(G) - G_ref).max() <= tol, (theta, phi is None)


# ---- the reference against 50 digits -----------------------------------------------------------------------------------
@pytest.mark.skipif(not sr.HAVE_MPMATH, reason="mpmath is not importable")
def test_long_double_code_equals_50_digits():
    """se3_exp, Jr^-1 and the long-double solve against mpmath at 50 digits: 1e-18 of the entries' scale
    (max(1, |rho|_inf) for the exponential, 1 + |phi|^2 / 12 for Jr^-1), i.e. nine long-double eps for expressions of a
    dozen operations; the solve to 8 eps_ld kappa |x|.  Angles on both sides of the series' switch at 0.1 included."""
    import mpmath
    rng = np.random.default_rng(50)
    worst = 0.0
    with mpmath.workdps(50):
        for theta in (0.0, 1e-9, 1e-6, 1e-3, 0.0999, 0.1, 0.1001, 0.5, 1.0, np.pi / 2, 2.69, 3.1, np.pi - 1e-8, np.pi, 4.7,
                      2 * np.pi, 7.0):
            for scale in (1.0, 100.0):
                phi = theta * sr.unit_axes(rng, 1)[0]
                rho = rng.normal(size=3)
                rho *= scale / np.abs(rho).max()
                xi = np.r_[rho, phi]
                diff = np.abs(sr.se3_exp(xi) - sr.mp_to_ld(mp_exp := sr.mp_se3_exp(xi))).max()
                assert mp_exp[3, 3] == 1
                worst = max(worst, float(diff) / scale)
                assert diff <= 1e-18 * scale, (theta, scale, float(diff))
            if theta <= np.pi:
                diff = np.abs(sr.jr_inv(phi) - sr.mp_to_ld(sr.mp_jr_inv(phi))).max()
                worst = max(worst, float(diff))
                assert diff <= 1e-18 * (1.0 + theta * theta / 12.0), (theta, float(diff))
        for cond in (1e2, 1e6, 1e10):
            Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
            A = (Q * np.geomspace(1.0, cond, 6)) @ Q.T
            A, b = 0.5 * (A + A.T), rng.normal(size=6)
            x = sr.solve(A, b)
            x_ld = sr._gauss(A.astype(LD), b.astype(LD))
            kappa = sr.condition_number(A)
            assert abs(kappa / cond - 1.0) <= 1e-3
            assert np.sqrt(f64((x - x_ld) @ (x - x_ld))) <= 8 * sr.LD_EPS * kappa * np.sqrt(f64(x @ x))
            # and the 50-digit solve leaves no residual a long double can show: |A x - b| <= 4 eps_ld |A| |x|
            assert np.abs(A.astype(LD) @ x - b).max() <= 4 * sr.LD_EPS * float(np.abs(A).sum(axis=1).max() * np.abs(x).max())
    print(f"worst |long double - 50 digits| / scale {worst:.2e}")


# ---- the exponential's device test has teeth ---------------------------------------------------------------------------
B_SERIES = [1 / 2, -1 / 24, 1 / 720, -1 / 40320, 1 / 3628800, -1 / 479001600, 1 / 87178291200, -1 / 20922789888000]
C_SERIES = [1 / 6, -1 / 120, 1 / 5040, -1 / 362880, 1 / 39916800, -1 / 6227020800, 1 / 1307674368000,
            -1 / 355687428096000]


def device_series(rho, phi, small, scale_pair=None, factor=1.0):
    """se3_exp_device's series branch restated in numpy over N inputs (the same Estrin grouping, products and sums
    rounded one by one where the device fuses them): (R N x 3 x 3, t N x 3).  scale_pair k: b_k and c_k times factor."""
    b, c = list(B_SERIES), list(C_SERIES)
    if scale_pair is not None:
        b[scale_pair] *= factor
        c[scale_pair] *= factor
    px, py, pz = rho.T
    rx, ry, rz = phi.T
    n2 = rx * rx + ry * ry + rz * rz
    z2 = n2 * n2
    z4 = z2 * z2
    pair = lambda s, k: n2 * s[k + 1] + s[k]
    B = z4 * (z2 * pair(b, 6) + pair(b, 4)) + (z2 * pair(b, 2) + pair(b, 0))
    C = z4 * (z2 * pair(c, 6) + pair(c, 4)) + (z2 * pair(c, 2) + pair(c, 0))
    A, cs = 1.0 - n2 * C, 1.0 - n2 * B
    bx, by, bz, ax, ay, az = B * rx, B * ry, B * rz, A * rx, A * ry, A * rz
    R = np.empty((len(n2), 3, 3))
    R[:, 0, 0], R[:, 1, 1], R[:, 2, 2] = bx * rx + cs, by * ry + cs, bz * rz + cs
    R[:, 0, 1], R[:, 1, 0] = bx * ry - az, bx * ry + az
    R[:, 0, 2], R[:, 2, 0] = bx * rz + ay, bx * rz - ay
    R[:, 1, 2], R[:, 2, 1] = by * rz - ax, by * rz + ax
    cd = C * (rx * px + ry * py + rz * pz)
    t = np.stack([A * px + (cd * rx + B * (ry * pz - rz * py)), A * py + (cd * ry + B * (rz * px - rx * pz)),
                  A * pz + (cd * rz + B * (rx * py - ry * px))], axis=1)
    return R, np.where(small[:, None], rho, t)


def worst_ratio(R, t, R_ref, t_ref, bound):
    """The device test's three comparisons as one figure: the largest |difference| / bound over R, t and R^T R - I."""
    orth = np.einsum("nki,nkj->nij", R, R) - np.eye(3)
    per_input = np.maximum.reduce([np.abs(f64(R.astype(LD) - R_ref)).max(axis=(1, 2)),
                                   np.abs(f64(t.astype(LD) - t_ref)).max(axis=1), np.abs(orth).max(axis=(1, 2))])
    return float((per_input / bound).max())


def test_exponential_bound_sees_every_coefficient_pair_up_to_five():
    """The device test's inputs that the series branch may take (|phi|^2 <= 0.25, the value 0.5 of the sweep included
    whichever way its square rounds) and its bound 4 eps max(1, |rho|_inf) (1 + |phi|), on a numpy restatement of the
    series: the intact series passes with a factor 2 to spare, and it fails with coefficient pair k (b_k, c_k) dropped,
    and with pair k off by 1 %, for every k <= 5.

    Measured: the intact series uses 0.25 of the bound; 1 % on pair 5 exceeds it 8.6 times, pair 5 dropped 862 times,
    pair 4 4.5e3 and 4.5e5 times, the lower pairs by more.  Pairs 6 and 7 are at or below what fp64 can show at
    |phi| <= 0.5: b_6 0.25^6 = 2.8e-15 enters R with |phi|^2 = 0.25 in front, 7e-16 of a bound of 1.3e-15, so pair 6
    dropped measures 1.18 x the bound (too near to it to assert), and pair 6 1 % off or pair 7 dropped or 1 % off leave
    the figure at 0.25.  Nothing is
    asserted about them: a wrong digit there costs no accuracy either."""
    rows = [(rho, phi, small) for name, rho, phi, small in sr.exp_sweep() if name != "angle"]
    rho, phi, small = (np.concatenate([r[k] for r in rows]) for k in range(3))
    assert (np.einsum("ni,ni->n", phi, phi) <= 0.25 * (1 + 4 * EPS)).all() and len(phi) > 3000
    R_ref, t_ref = sr.se3_exp_many(rho, phi, small)
    bound = sr.exp_bound(rho, phi)
    intact = worst_ratio(*device_series(rho, phi, small), R_ref, t_ref, bound)
    print(f"intact series: {intact:.3f} of the bound")
    assert intact <= 0.5
    for k in range(6):
        dropped = worst_ratio(*device_series(rho, phi, small, k, 0.0), R_ref, t_ref, bound)
        scaled = worst_ratio(*device_series(rho, phi, small, k, 1.01), R_ref, t_ref, bound)
        print(f"pair {k}: dropped {dropped:.3g} x the bound, 1 % off {scaled:.3g} x")
        assert dropped > 1.0 and scaled > 1.0, (k, dropped, scaled)
