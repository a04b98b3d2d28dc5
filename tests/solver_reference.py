"""The reference of the solver-domain tests: se3ToSE3, Log, Jr^-1, the pose prior's chart and a 6 x 6 solve in extended
precision (numpy.longdouble with a 64-bit significand), plus the inputs the CPU and the GPU test share.  Not a test module.

Written from the textbook closed forms, independently of eskf_lio_amd/csrc/vgicp_math.h and of tests/prior_reference.py:
  R   = cos(th) I + 2 sin^2(th/2) a a^T + sin(th) [a]x                       (no 1 - cos: nothing cancels)
  J_l = A I + B [phi]x + C phi phi^T,  A = sin th / th,  B = 2 sin^2(th/2) / th^2,  C = (th - sin th) / th^3
  c   = (1 - (th/2) cot(th/2)) / th^2  of  Jr^-1(phi) = I + [phi]x / 2 + c [phi]x^2
C and c cancel near zero (th - sin th loses 6 / th^2, 1 - (th/2) cot(th/2) loses 12 / th^2), so below SERIES_BELOW = 0.1
both take their Taylor series (ten terms: truncated below 1e-30); at 0.1 the closed forms lose a factor of 600 and 1200
of the long double's 1.1e-19, in terms that themselves carry th^2 / 6 and th^2 / 12 of the result: below 1e-19 of it.
Angles and axes go in as they are known (theta, unit axis): nothing here recovers an angle from a rounded matrix, except
so3_log, which is there for matrices that are given as matrices.

The project's se3ToSE3 is the reference implementation's, which sets J_l = I while sqrt(|phi|^2) < 1e-6 (in fp64); the
caller says on which side an input lies (small_identity), since that is a property of the fp64 input, not of the map.

Where mpmath is importable the same quantities are also available at 50 digits (mp_*), straight closed forms with limits
at zero only, for checking the long-double code itself; solve() then uses mpmath's LU at 50 digits.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
LD_EPS = float(np.finfo(LD).eps)
SERIES_BELOW = 0.1
SMALL_ANGLE2 = float.fromhex("0x1.19799812dea10p-40")   # smallest double whose square root rounds to >= 1e-6

try:
    import mpmath
    HAVE_MPMATH = True
except ImportError:                                       # pragma: no cover
    mpmath = None
    HAVE_MPMATH = False


def unavailable_reason():
    """None where this reference is finer than fp64 on this machine, else why not (the tests skip with it).  The
    arithmetic is long double throughout; mpmath, where importable, checks it and carries the solve."""
    if LD_EPS < 2e-19:
        return None
    return f"numpy.longdouble has eps {LD_EPS:.1e} here, not below 2e-19: no extended precision to compute the reference in"


PI = 4 * np.arctan(LD(1))


def _factorial(n):
    out = LD(1)
    for k in range(2, n + 1):
        out *= k
    return out


def hat(v):
    v = np.asarray(v, dtype=LD)
    z = LD(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=LD)


def so3_exp(theta, axis):
    """Rotation by theta about the unit vector axis."""
    th, a = LD(theta), np.asarray(axis, dtype=LD)
    h = np.sin(th / 2)
    return np.cos(th) * np.eye(3, dtype=LD) + 2 * h * h * np.outer(a, a) + np.sin(th) * hat(a)


def jl_coefficients(th):
    """(A, B, C) of J_l = A I + B [phi]x + C phi phi^T at the angle th >= 0."""
    th = LD(th)
    n2 = th * th
    if th < SERIES_BELOW:
        A = sum((-1) ** k * n2 ** k / _factorial(2 * k + 1) for k in range(10))
        B = sum((-1) ** k * n2 ** k / _factorial(2 * k + 2) for k in range(10))
        C = sum((-1) ** k * n2 ** k / _factorial(2 * k + 3) for k in range(10))
        return A, B, C
    h = np.sin(th / 2)
    return np.sin(th) / th, 2 * h * h / n2, (th - np.sin(th)) / (n2 * th)


def se3_exp(xi, small_identity=False):
    """se3ToSE3 of xi = [rho; phi] (fp64 or long double, taken as exact): 4 x 4 long double.  small_identity: t = rho."""
    xi = np.asarray(xi, dtype=LD)
    rho, phi = xi[:3], xi[3:]
    th = np.sqrt(phi @ phi)
    A, B, C = jl_coefficients(th)
    K = hat(phi)
    T = np.eye(4, dtype=LD)
    # R = I + A [phi]x + B [phi]x^2, written with phi phi^T so that the diagonal is cos th + B phi_i^2
    T[:3, :3] = (1 - th * th * B) * np.eye(3, dtype=LD) + B * np.outer(phi, phi) + A * K
    T[:3, 3] = rho if small_identity else A * rho + B * (K @ rho) + C * phi * (phi @ rho)
    return T


def se3_exp_many(rho, phi, small_identity):
    """se3_exp over N inputs at once: rho, phi N x 3 (fp64, exact), small_identity N bools -> (R N x 3 x 3, t N x 3)."""
    rho, phi = np.asarray(rho, dtype=LD), np.asarray(phi, dtype=LD)
    n2 = np.einsum("ni,ni->n", phi, phi)
    th = np.sqrt(n2)
    coeff = np.array([jl_coefficients(v) for v in th], dtype=LD)
    A, B, C = coeff[:, 0], coeff[:, 1], coeff[:, 2]
    eye = np.eye(3, dtype=LD)
    K = np.zeros((len(th), 3, 3), dtype=LD)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -phi[:, 2], phi[:, 1], phi[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -phi[:, 0], -phi[:, 1], phi[:, 0]
    R = ((1 - n2 * B)[:, None, None] * eye + B[:, None, None] * np.einsum("ni,nj->nij", phi, phi) + A[:, None, None] * K)
    t = (A[:, None] * rho + B[:, None] * np.einsum("nij,nj->ni", K, rho)
         + (C * np.einsum("ni,ni->n", phi, rho))[:, None] * phi)
    t = np.where(np.asarray(small_identity, dtype=bool)[:, None], rho, t)
    return R, t


def so3_log(M):
    """Rotation vector of a rotation matrix given as a matrix, |phi| <= pi.  Away from pi the axis is vee(M - M^T);
    for cos <= -0.9 it is the column of the symmetric part (M + M^T) / 2 - cos I = (1 - cos) a a^T with the largest
    diagonal, normalised, signed by vee(M - M^T) (left as it is where that sign is zero: at pi both are the Log)."""
    M = np.asarray(M, dtype=LD)
    v = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]], dtype=LD) / 2
    s, c = np.sqrt(v @ v), (M[0, 0] + M[1, 1] + M[2, 2] - 1) / 2
    th = np.arctan2(s, c)
    if c > LD(-0.9):
        return v * (th / s) if s > 0 else v.copy()
    P = (M + M.T) / 2 - c * np.eye(3, dtype=LD)
    a = P[:, int(np.argmax(np.diag(P)))]
    a = a / np.sqrt(a @ a)
    if v @ a < 0:
        a = -a
    return th * a


def jr_inv_coefficient(th):
    """c(theta) of Jr^-1."""
    th = LD(th)
    n2 = th * th
    if th < SERIES_BELOW:
        # sum |B_2k| theta^(2k - 2) / (2k)!, k = 1 .. 10 (Bernoulli numbers 1/6, 1/30, 1/42, 1/30, 5/66, 691/2730, 7/6,
        # 3617/510, 43867/798, 174611/330)
        bern = ((1, 6), (1, 30), (1, 42), (1, 30), (5, 66), (691, 2730), (7, 6), (3617, 510), (43867, 798), (174611, 330))
        return sum(LD(p) / LD(q) / _factorial(2 * k) * n2 ** (k - 1) for k, (p, q) in enumerate(bern, start=1))
    return (1 - (th / 2) * np.cos(th / 2) / np.sin(th / 2)) / n2


def jr_inv(phi, c_scale=1.0):
    """Jr^-1(phi) = I + [phi]x / 2 + c [phi]x^2.  c_scale != 1 falsifies c (for the tests that prove they see it)."""
    phi = np.asarray(phi, dtype=LD)
    K = hat(phi)
    return np.eye(3, dtype=LD) + K / 2 + LD(c_scale) * jr_inv_coefficient(np.sqrt(phi @ phi)) * (K @ K)


def chart(T0, T, phi=None, c_scale=1.0):
    """(d (6), G (6 x 6)) of the pose prior at T against T0: d = [t - t0; phi], G = [I, -[t]x; 0, Jr^-1(phi) R^T].
    phi = Log(R0^T R) where the caller knows it by construction, else so3_log of the product."""
    T0, T = np.asarray(T0, dtype=LD), np.asarray(T, dtype=LD)
    if phi is None:
        phi = so3_log(T0[:3, :3].T @ T[:3, :3])
    phi = np.asarray(phi, dtype=LD)
    d = np.concatenate([T[:3, 3] - T0[:3, 3], phi])
    G = np.zeros((6, 6), dtype=LD)
    G[:3, :3] = np.eye(3, dtype=LD)
    G[:3, 3:] = -hat(T[:3, 3])
    G[3:, 3:] = jr_inv(phi, c_scale) @ T[:3, :3].T
    return d, G


def solve(A, b):
    """x of A x = b for a 6 x 6 (any n x n) system whose entries are taken as exact: mpmath's LU at 50 digits where
    mpmath is importable, else Gaussian elimination with partial pivoting and two rounds of refinement in long double
    (error ~ kappa x 1e-19 before the refinement).  Returns long double."""
    A, b = np.asarray(A, dtype=LD), np.asarray(b, dtype=LD)
    if HAVE_MPMATH:
        with mpmath.workdps(50):
            x = mpmath.lu_solve(_to_mp(A), _to_mp(b.reshape(-1, 1)))
            return np.array([_from_mp(x[i]) for i in range(len(b))], dtype=LD)
    x = _gauss(A, b)
    for _ in range(2):
        x = x + _gauss(A, b - A @ x)
    return x


def _gauss(A, b):
    n = len(b)
    M = np.concatenate([A, b.reshape(n, 1)], axis=1).astype(LD)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        M[[k, p]] = M[[p, k]]
        for i in range(k + 1, n):
            M[i, k:] -= (M[i, k] / M[k, k]) * M[k, k:]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (M[i, n] - M[i, i + 1:n] @ x[i + 1:]) / M[i, i]
    return x


def inverse(A):
    """A^-1 of a matrix whose entries are taken as exact, rounded to long double: mpmath at 50 digits where importable,
    else column by column through solve()."""
    A = np.asarray(A, dtype=LD)
    if HAVE_MPMATH:
        with mpmath.workdps(50):
            return mp_to_ld(mpmath.inverse(_to_mp(A)))
    return np.array([solve(A, e) for e in np.eye(A.shape[0], dtype=LD)], dtype=LD).T


def condition_number(A, inv=None):
    """||A||_2 ||A^-1||_2 of a symmetric fp64 matrix, the inverse by inverse(): both norms are LARGEST eigenvalues, which
    fp64's eigvalsh returns to a few eps relative, whatever the condition (the smallest of A itself it does not)."""
    A = np.asarray(A, dtype=np.float64)
    inv = inverse(A) if inv is None else inv
    scale = np.abs(inv).max()
    inv64 = (inv / scale).astype(np.float64)
    norm, norm_inv = np.abs(np.linalg.eigvalsh(A)).max(), np.abs(np.linalg.eigvalsh(0.5 * (inv64 + inv64.T))).max()
    return float(norm * norm_inv * float(scale))


# ---- 50 digits ---------------------------------------------------------------------------------------------------------
def _to_mp(a):
    """long double array -> mpmath matrix, exactly (a long double is hi + lo of two doubles)."""
    a = np.atleast_2d(np.asarray(a, dtype=LD))
    out = mpmath.matrix(a.shape[0], a.shape[1])
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            hi = float(a[i, j])
            out[i, j] = mpmath.mpf(hi) + mpmath.mpf(float(a[i, j] - LD(hi)))
    return out


def _from_mp(v):
    hi = float(v)
    return LD(hi) + LD(float(v - mpmath.mpf(hi)))


def mp_to_ld(M):
    return np.array([[_from_mp(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], dtype=LD)


def _mp_hat(v):
    return mpmath.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def mp_se3_exp(xi):
    """se3ToSE3 (without the 1e-6 branch) at the working precision of mpmath: 4 x 4 mpmath matrix.  Closed forms, the
    limits 1, 1/2, 1/6 at phi = 0."""
    rho, phi = mpmath.matrix([mpmath.mpf(float(v)) for v in xi[:3]]), mpmath.matrix([mpmath.mpf(float(v)) for v in xi[3:]])
    th = mpmath.sqrt(sum(p * p for p in phi))
    K = _mp_hat(phi)
    if th == 0:
        A, B, C = mpmath.mpf(1), mpmath.mpf(1) / 2, mpmath.mpf(1) / 6
    else:
        A, B, C = mpmath.sin(th) / th, (1 - mpmath.cos(th)) / th ** 2, (th - mpmath.sin(th)) / th ** 3
    R = mpmath.eye(3) + A * K + B * K * K
    t = A * rho + B * (K * rho) + C * phi * (phi.T * rho)[0]
    T = mpmath.eye(4)
    for i in range(3):
        for j in range(3):
            T[i, j] = R[i, j]
        T[i, 3] = t[i]
    return T


def mp_jr_inv(phi):
    phi = mpmath.matrix([mpmath.mpf(float(v)) for v in phi])
    th = mpmath.sqrt(sum(p * p for p in phi))
    c = mpmath.mpf(1) / 12 if th == 0 else 1 / th ** 2 - (1 + mpmath.cos(th)) / (2 * th * mpmath.sin(th))
    K = _mp_hat(phi)
    return mpmath.eye(3) + K / 2 + c * K * K


# ---- shared inputs: the exponential over its domain --------------------------------------------------------------------
def unit_axes(rng, n):
    a = rng.normal(size=(n, 3))
    return a / np.linalg.norm(a, axis=1)[:, None]


def exp_sweep():
    """The inputs of the exponential's domain test, the same for the device test and for the CPU test that proves the
    bound has teeth: a list of (branch name, rho N x 3, phi N x 3, small_identity N bools), all fp64.

    |phi|: 40 log-spaced values from 1e-9 to 0.5; both sides of kSmallAngle2 and of n2 = 0.25 by nextafter on n2 with
    phi along one axis, so that n2 = phi_x^2 is what the device computes; 0.5 ... pi in steps of 0.25, pi, 3 pi / 2,
    2 pi, 7.0.  20 random axes per angle (the one-axis cases: the three coordinate axes, both signs).  rho: a random
    direction scaled to |rho|_inf = 0.1, 1 and 100, and rho = 0.  The branch is by the fp64 |phi|^2: 'identity'
    (t = rho) below kSmallAngle2, 'series' up to 0.25, 'angle' above; the random-axis angles keep clear of both switches
    by more than 1e-6 relative, so the name does not depend on how |phi|^2 is rounded — except the sweep's last value,
    0.5 itself, which is named 'switch': either branch may take it and both must meet the bound."""
    rng = np.random.default_rng(20260)
    cases = []

    def add(name, phis, small):
        phis = np.asarray(phis, dtype=np.float64)
        for scale in (0.1, 1.0, 100.0, 0.0):
            rho = rng.normal(size=phis.shape)
            rho *= scale / np.abs(rho).max(axis=1)[:, None]
            cases.append((name, rho, phis, np.full(len(phis), small)))

    for mag in np.geomspace(1e-9, 0.5, 40):
        n2 = mag * mag
        assert abs(n2 / SMALL_ANGLE2 - 1.0) > 1e-6
        name = "identity" if n2 < SMALL_ANGLE2 else "switch" if mag >= 0.5 else "series"
        add(name, mag * unit_axes(rng, 20), name == "identity")
    signed = np.concatenate([np.eye(3), -np.eye(3)])
    below = np.sqrt(SMALL_ANGLE2)                     # the largest double whose square rounds below kSmallAngle2 ...
    while below * below >= SMALL_ANGLE2:
        below = np.nextafter(below, 0.0)
    above = np.nextafter(below, 1.0)                  # ... and its neighbour, whose square does not
    assert below * below < SMALL_ANGLE2 <= above * above and np.sqrt(below * below) < 1e-6 <= np.sqrt(above * above)
    add("identity", below * signed, True)
    add("series", above * signed, False)
    above = np.nextafter(0.5, 1.0)
    assert 0.5 * 0.5 == 0.25 < above * above
    add("series", 0.5 * signed, False)
    add("angle", above * signed, False)
    for mag in list(np.arange(0.75, np.pi, 0.25)) + [np.pi, 1.5 * np.pi, 2.0 * np.pi, 7.0]:
        add("angle", mag * unit_axes(rng, 20), False)
    return cases


def exp_bound(rho, phi):
    """4 eps max(1, |rho|_inf) (1 + |phi|) per input: the bound on every entry of R, of t and of R^T R - I."""
    return 4.0 * EPS * np.maximum(1.0, np.abs(rho).max(axis=1)) * (1.0 + np.linalg.norm(phi, axis=1))


# ---- shared inputs: the fast solve towards its guard -------------------------------------------------------------------
SOLVE_CONDITIONS = tuple(10.0 ** (0.5 * k) for k in range(16, 31))        # 1e8 ... 1e15, half a decade apart


def solve_sweeps(systems=10):
    """[(kind, [(nominal condition, A 6 x 6 symmetric fp64, b), ...]), ...]: `systems` sweeps of each kind, every sweep
    one family of systems along SOLVE_CONDITIONS.
      'orthogonal'  Q diag(geomspace(1, cond, 6)) Q^T with one random orthogonal Q per sweep
      'graded'      A_data + diag(lambda, lambda, lambda, 0, 0, 0): A_data one random SPD matrix per sweep with
                    eigenvalues 1e3 ... 2e4, lambda = 1e3 cond (1e18 at the end): a prior that pins the translation."""
    rng = np.random.default_rng(515)
    out = []
    for kind in ("orthogonal", "graded"):
        for _ in range(systems):
            Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
            b = rng.normal(size=6)
            sweep = []
            for cond in SOLVE_CONDITIONS:
                if kind == "orthogonal":
                    A = (Q * np.geomspace(1.0, cond, 6)) @ Q.T
                else:
                    A = (Q * np.geomspace(1e3, 2e4, 6)) @ Q.T + np.diag([1e3 * cond] * 3 + [0.0] * 3)
                sweep.append((cond, 0.5 * (A + A.T), b.copy()))
            out.append((kind, sweep))
    return out
