"""The reference of the match-term tests: ONE correspondence's contribution to a round (accumulate_match, inverse3_cofactor,
rcp_newton and robust_weight of eskf_lio_amd/csrc/vgicp_kernels.hip, the cost and squared-error slots of evaluate_kernel)
in 60-digit arithmetic (mpmath), the bound on the device's distance from it, and the inputs the CPU and the GPU test
share.  Not a test module.

THE TERM.  Given the fp64 pose (R, t), the fp64 point AS TRANSFORMED p = fl(R x + t) (oracle.transform's p; DESIGN.md
promises the device's bits equal it in round 0, so taking p as given isolates the term from the transform), the scan
covariance C (9 doubles, column-major, NOT assumed symmetric), the voxel's mean mu and covariance C_voxel:
    S = R C R^T + C_voxel,  W = S^-1 (the general 3 x 3 inverse, never symmetrised),  e = p - mu,  J = [I | -[p]x]
    29 values: the 21 lower-triangle entries of J^T W J row by row, the 6 of J^T W e, e^T W e, |e|^2.
Every input is an fp64 number taken as exact; nothing is rounded before the 29 results.  Long double would not do: its
own error in W would be kappa^2 x 1e-19, which at kappa = 1e5 is fp64's.

THE BOUND (u = 2^-53, first order in u; counted, not fitted).  l1 >= l2 >= l3 are the magnitudes of S's eigenvalues,
rho = l1^2 / (l2 l3).  For a symmetric S every |S_ij| <= l1 and every |W_ij| <= 1 / l3 =: w; the derivation is written
for that case and the two places where it uses these facts take the actual maxima instead (g and w below), so that it
also holds for the asymmetric groups:
    m = g l1 bounds every |S_ij| and every entry of |R| |C| |R|^T,  g = max(1, those maxima / l1)
    w = max(1 / l3, max |W_ij|),  r = max(rho, l1 w)                          (symmetric S: g = 1, w = 1 / l3, r = rho)
  S itself.  R C and (R C) R^T are 3-term dot products (3 u each against sum |a_i b_i|, with or without contraction):
      6 u (|R| |C| |R|^T)_ij, plus one addition of C_voxel: |dS_ij| <= 7 m u.  W moves by -W dS W, entrywise at most
      9 w^2 7 m u = 63 u (l1 w) g w                                                                             -> 63
  Cofactors.  a b - c d as two products and a difference, or one product and one FMA: <= 2 u (|a b| + |c d|) <= 4 m^2 u.
  det = c00 S00 + c10 S10 + c20 S20: the cofactors' errors 3 x 4 m^2 u x m, the dot product's own 3 u sum |c_i S_i|
      <= 3 u x 3 x 2 m^3: 30 m^3 u, relative to |det| = l1 l2 l3: 30 g^3 rho u, times |W_ij| <= w                -> 30
  The reciprocal (v_rcp_f64 + one third-order step, at most 1 ulp = 2 u) and the product c_ij x (1 / det) (u)    ->  3
  The adjugate entry itself: 4 m^2 u / |det| = 4 g^2 u l1 / (l2 l3) <= 4 g^2 u rho / l1 <= 4 g^2 u rho w         ->  4
      B_W = 100 u g^3 r w                      on every entry of W   (symmetric S: 100 u rho / l3; COST_W = 100)
  Then, with |p|_1 and |e|_1 the 1-norms and every |W_ij| <= w (a difference of two products: 2 u against the sum of
  their magnitudes; a 3-term dot product: 3 u; e = p - mu is one rounding, relative u per component):
      slots 0-5    W                                   B_W
      Q = [p]x W   rows 3-5, columns 0-2               |p|_1 (B_W + 2 u w)
      rows 3-5, columns 3-5   Q (-[p]x)                |p|_1^2 (B_W + 4 u w)
      slots 21-23  W e                                 |e|_1 (B_W + 4 u w)
      slots 24-26  Q e                                 |e|_1 |p|_1 (B_W + 6 u w)
      cost         e . (W e)                           |e|_1^2 (B_W + 8 u w)
      |e|^2        three squares of rounded e_i        5 u |e|^2
  The weighted row (include/vgicp_hip_robust.h): w_ref x (the plain bound) + 4 u |w_ref x (the reference slot)|: the
  weight's own roundings (one sum or product, the reciprocal or reciprocal square root, c^2 x ., W x w).

THE SWEEP (sweep()): one small map (VOXEL = 1 m, about 60 voxels whose keys, means and covariances are set explicitly, so
a mean lies wherever the case wants it), and named groups, each ONE scan point (x, C) with up to 64 poses that carry x to
the centre of a chosen voxel (t = centre - R x), so the transform's rounding cannot move a key.  Axes: scale, the
conditioning of S, the indefinite class, asymmetry, distance and |e|, rotations, and anchors whose 29 values are exactly
representable.  weight_groups(): the inputs of the robust-weight test in the same form, with the robust settings.
"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

try:
    import mpmath
    from mpmath import mp, mpf
    HAVE_MPMATH = True
except ImportError:                                       # pragma: no cover
    mpmath = None
    HAVE_MPMATH = False

U = 2.0 ** -53
DPS = 60
VOXEL = 1.0
COST_W = 100                  # the counted constant of B_W (derivation above)
NONE, HUBER, CAUCHY = 0, 1, 2
SLOTS = [(r, c) for r in range(6) for c in range(r + 1)]          # the row's order of the 21 lower-triangle entries


def unavailable_reason():
    """None where the reference can be computed, else why not (the tests skip with it)."""
    if HAVE_MPMATH:
        return None
    return "mpmath is not importable: no arithmetic finer than long double to compute the match term's reference in"


def cm(M):
    """3 x 3 (row, col) numpy -> the ABI's 9 doubles, column-major."""
    return np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(9)


def from_cm(v):
    return np.asarray(v, dtype=np.float64).reshape(3, 3).T.copy()


def pose4(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def transform(R, t, x):
    """Open3D's homogeneous product as oracle.transform and the device's transform_point evaluate it: left to right, no
    contraction (numpy scalars never fuse)."""
    R, t, x = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return np.array([((R[r, 0] * x[0] + R[r, 1] * x[1]) + R[r, 2] * x[2]) + t[r] for r in range(3)])


# ---- the reference -----------------------------------------------------------------------------------------------------
def _mp3(M):
    return mpmath.matrix([[mpf(float(M[r, c])) for c in range(3)] for r in range(3)])


@dataclass
class Term:
    values: list                 # 29 mpf: 21 + 6 + cost + |e|^2
    l: np.ndarray                # magnitudes of S's eigenvalues, descending
    rho: float
    w_max: float                 # max |W_ij|
    s_max: float                 # max over |S_ij| and (|R| |C| |R|^T)_ij
    p1: float
    e1: float
    e2: float                    # |e|^2

    @property
    def f64(self):
        return np.array([float(v) for v in self.values])

    @property
    def raw(self):
        """e^T W e, the robust round's raw residual."""
        return self.values[27]

    def bounds(self):
        """The 29 bounds of the module docstring."""
        l1, l3 = float(self.l[0]), float(self.l[2])
        g = max(1.0, self.s_max / l1)
        w = max(1.0 / l3, self.w_max)
        r = max(self.rho, l1 * w)
        bw = COST_W * U * g ** 3 * r * w
        out = np.empty(29)
        for k, (row, col) in enumerate(SLOTS):
            out[k] = bw if row < 3 else self.p1 * (bw + 2 * U * w) if col < 3 else self.p1 ** 2 * (bw + 4 * U * w)
        out[21:24] = self.e1 * (bw + 4 * U * w)
        out[24:27] = self.e1 * self.p1 * (bw + 6 * U * w)
        out[27] = self.e1 ** 2 * (bw + 8 * U * w)
        out[28] = 5 * U * self.e2
        return out

    def differences(self, got):
        """|got - reference| for 29 fp64 values, the difference formed at the reference's precision."""
        with mp.workdps(DPS):
            return np.array([float(abs(mpf(float(g)) - v)) for g, v in zip(got, self.values)])


def term(R, p, C9, mu, Cv9):
    """The reference of one term.  R 3 x 3 (row, col) numpy; p, mu 3; C9, Cv9 the ABI's column-major 9 doubles."""
    R, C, Cv = np.asarray(R, dtype=np.float64), from_cm(C9), from_cm(Cv9)
    p, mu = np.asarray(p, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    with mp.workdps(DPS):
        Rm = _mp3(R)
        S = Rm * _mp3(C) * Rm.T + _mp3(Cv)
        W = mpmath.inverse(S)
        pm = [mpf(float(v)) for v in p]
        e = mpmath.matrix([pm[k] - mpf(float(mu[k])) for k in range(3)])
        J = mpmath.zeros(3, 6)
        hat = [[0, -pm[2], pm[1]], [pm[2], 0, -pm[0]], [-pm[1], pm[0], 0]]
        for r in range(3):
            J[r, r] = 1
            for c in range(3):
                J[r, 3 + c] = -hat[r][c]
        JTW = J.T * W
        H, b = JTW * J, JTW * e
        values = [H[r, c] for r, c in SLOTS] + [b[k] for k in range(6)] + [(e.T * W * e)[0], (e.T * e)[0]]
        eig = mpmath.eig(S, left=False, right=False)
        l = np.sort(np.array([float(abs(v)) for v in eig]))[::-1]
        w_max = max(float(abs(W[r, c])) for r in range(3) for c in range(3))
        s_abs = max(float(abs(S[r, c])) for r in range(3) for c in range(3))
        e1, e2 = float(sum(abs(v) for v in e)), float((e.T * e)[0])
    a_abs = float((np.abs(R) @ np.abs(C) @ np.abs(R).T).max())
    return Term(values, l, float(l[0] ** 2 / (l[1] * l[2])), w_max, max(s_abs, a_abs), float(np.abs(p).sum()), e1, e2)


def weight(raw, kernel, c, gate):
    """The header's formulas on the reference's raw residual (mpf): (weight, mpf; counted).  d^2 = max(raw, 0); a gate
    g > 0 rejects !(raw <= g); Huber w = 1 if d^2 <= c^2 else c / sqrt(d^2); Cauchy w = 1 / (1 + d^2 / c^2)."""
    with mp.workdps(DPS):
        d2 = raw if raw > 0 else mpf(0)
        c2 = mpf(float(c)) ** 2
        if kernel == HUBER:
            w = mpf(1) if d2 <= c2 else mpf(float(c)) / mpmath.sqrt(d2)
        elif kernel == CAUCHY:
            w = 1 / (1 + d2 / c2)
        else:
            w = mpf(1)
        if gate > 0.0 and not raw <= mpf(float(gate)):
            w = mpf(0)
        return w, bool(w > 0)


@dataclass
class WeightedRow:
    w: float                     # the reference weight, rounded
    counted: bool                # w_ref > 0
    values: list                 # 27 mpf: w_ref x (the reference slot)
    bounds: np.ndarray           # w_ref x (the plain bound) + 4 u |w_ref x (the reference slot)|
    representable: bool          # the weight and all 27 products are fp64 numbers

    def differences(self, got):
        with mp.workdps(DPS):
            return np.array([float(abs(mpf(float(g)) - v)) for g, v in zip(got, self.values)])

    def ratios(self, got):
        """|got - reference| / bound per slot; a difference where the bound is zero is infinitely far out."""
        d = self.differences(got)
        return np.where(self.bounds > 0, d / np.where(self.bounds > 0, self.bounds, 1.0), np.where(d > 0, np.inf, 0.0))


def weighted_row(t, kernel, c, gate):
    """The weighted row's reference for the term t under (kernel, c, gate)."""
    with mp.workdps(DPS):
        w, counted = weight(t.raw, kernel, c, gate)
        values = [w * v for v in t.values[:27]]
        wf = float(w)
        bounds = wf * t.bounds()[:27] + 4 * U * np.array([float(abs(v)) for v in values])
        representable = mpf(wf) == w and all(mpf(float(v)) == v for v in values)
    return WeightedRow(wf, counted, values, bounds, representable)


# ---- the inputs --------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    R: np.ndarray
    t: np.ndarray
    voxel: int                   # index into the map's arrays
    p: np.ndarray                # transform(R, t, x)
    label: str = ""

    @property
    def pose(self):
        return pose4(self.R, self.t)


@dataclass
class Group:
    name: str
    axis: str                    # scale / conditioning / indefinite / asymmetry / distance / anchor / weight
    x: np.ndarray
    C9: np.ndarray
    cases: list = field(default_factory=list)
    exact: bool = False          # every one of the 29 values is exactly representable: the device must return it with ==
    robust: tuple = ()           # weight groups: the (kernel, c, gate) settings the cases are run under


@dataclass
class Map:
    keys: list = field(default_factory=list)
    means: list = field(default_factory=list)
    covs: list = field(default_factory=list)      # column-major 9

    def add(self, key, mean, Cv):
        key = tuple(int(k) for k in key)
        assert key not in self.keys, key
        self.keys.append(key)
        self.means.append(np.asarray(mean, dtype=np.float64))
        self.covs.append(cm(Cv))
        return len(self.keys) - 1

    def centre(self, v):
        return (np.array(self.keys[v], dtype=np.float64) + 0.5) * VOXEL

    def arrays(self):
        return (np.array(self.keys, dtype=np.int32), np.array(self.means), np.array(self.covs))


def axis_rotation(axis, angle):
    """Rodrigues in fp64: the matrix as it goes to the device (cos(pi / 2) is 6e-17 there, not 0)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(angle) * np.eye(3) + (1 - np.cos(angle)) * np.outer(a, a) + np.sin(angle) * K


def random_rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q if np.linalg.det(Q) > 0 else -Q


def sym(M):
    return 0.5 * (M + M.T)                       # bitwise symmetric: such a scan is read from nine planes


def fixed_rotations():
    out = [("identity", np.eye(3))]
    for k, name in enumerate("xyz"):
        for angle, tag in ((0.5 * np.pi, "pi/2"), (np.pi, "pi")):
            out.append((f"{name} {tag}", axis_rotation(np.eye(3)[k], angle)))
    return out


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _case(vmap, x, R, voxel, label="", target=None):
    """The pose that carries x to `target` (default: the voxel's centre) under R; asserts the key."""
    target = vmap.centre(voxel) if target is None else np.asarray(target, dtype=np.float64)
    t = target - R @ x
    p = transform(R, t, x)
    assert tuple(np.floor(p / VOXEL).astype(int)) == vmap.keys[voxel], (label, p, vmap.keys[voxel])
    return Case(np.array(R, dtype=np.float64), t, voxel, p, label)


WEIGHT_KEY = (-1, -1, -1)          # the weight sweep's voxel: mean at the origin, p = t between -0.45 and 0 per component


def _near_keys():
    """Keys within two voxels of the origin in a fixed shuffled order, without the ones DISTANCES and WEIGHT_KEY name."""
    taken = {k for _, ks in DISTANCES for k in ks} | {WEIGHT_KEY}
    keys = [(i, j, k) for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3) if (i, j, k) not in taken]
    order = np.random.default_rng(7).permutation(len(keys))
    return [keys[i] for i in order]


SCALES = ((1e-8, 1e-8), (1e-4, 1e-4), (1.0, 1.0), (1e4, 1e4), (1e-6, 1.0), (1.0, 1e-6))     # (C, C_voxel)
DECADES = tuple(10.0 ** k for k in range(11))                                               # rho of the conditioning groups
NORMAL_EIGENVALUES = (5e-3, 1e-6, -1e-6, -5e-3)                                             # of S, the indefinite class
ASYMMETRIES = (1e-7, 1e-2, 0.7)                                                             # c01 - c10
DISTANCES = (("0", ((0, 0, 0),)),                                                            # |p|: one voxel per |e|
             ("1", ((0, -1, 0), (-1, 0, 0), (0, 0, -1), (-1, -1, 0))),
             ("100", tuple((57 + j, -58, 57) for j in range(4))),
             ("1e4", tuple((5773 + j, -5774, 5773) for j in range(4))))
RESIDUALS = (0.0, 1e-9, 0.1, 1.0)                                                           # |e|: 1.0 is a whole voxel


def sweep():
    """(Map, [Group]) — the module docstring's sweep.  Deterministic, built once."""
    return _build()[:2]


@lru_cache(maxsize=1)
def _build():
    rng = np.random.default_rng(20270)
    vmap, groups, free = Map(), [], _near_keys()
    rotations = fixed_rotations()
    randoms = [(f"random {k}", random_rotation(rng)) for k in range(20)]
    plate = np.diag([1.0, 1.0, 1e-2])

    def regularised():
        Q = random_rotation(rng)
        return sym(Q @ plate @ Q.T)

    V0 = regularised()

    # scale: C and C_voxel scaled, alike and mismatched; every rotation
    scale_voxel = {}
    for s in sorted({sv for _, sv in SCALES}):
        key = free.pop()
        scale_voxel[s] = vmap.add(key, (np.array(key) + 0.5) * VOXEL - 0.1 * _unit(rng), s * V0)
    for sc, sv in SCALES:
        g = Group(f"scale C {sc:g} C_voxel {sv:g}", "scale", rng.uniform(-3, 3, size=3), cm(sc * regularised()))
        g.cases = [_case(vmap, g.x, R, scale_voxel[sv], name) for name, R in rotations + randoms]
        groups.append(g)

    # conditioning: S = U diag(d) U^T with R C R^T = U diag(a) U^T and C_voxel = U diag(d - a) U^T, so that S itself
    # is ill-conditioned and both summands share its axes; one small eigenvalue (1, 1, 1 / rho), two (1, s, s), s^2 = 1 / rho
    Uc = random_rotation(rng)
    for shape in ("one small", "two small"):
        a = np.array([0.5, 0.5, 0.5e-10]) if shape == "one small" else np.array([0.5, 0.5e-5, 0.5e-5])
        voxels = []
        for rho in DECADES:
            d = np.array([1.0, 1.0, 1.0 / rho]) if shape == "one small" else np.array([1.0, rho ** -0.5, rho ** -0.5])
            assert (d - a > 0).all()
            key = free.pop()
            voxels.append(vmap.add(key, (np.array(key) + 0.5) * VOXEL - 0.1 * _unit(rng), sym(Uc @ np.diag(d - a) @ Uc.T)))
        for replica in range(2):
            Rg = random_rotation(rng)
            g = Group(f"conditioning, {shape}, {replica}", "conditioning", rng.uniform(-3, 3, size=3),
                      cm(sym(Rg.T @ Uc @ np.diag(a) @ Uc.T @ Rg)))
            g.cases = [_case(vmap, g.x, Rg, v, f"rho {rho:g}") for v, rho in zip(voxels, DECADES)]
            groups.append(g)

    # the indefinite class: C = Q diag(1, 1, -1e-2) Q^T as the scan preparation can return it, against a planar C_voxel
    # with the same normal; e along the normal and across it; rotations about the normal keep the alignment
    Un = random_rotation(rng)
    normal, across = Un[:, 2], Un[:, 0]
    voxels = []
    for lam in NORMAL_EIGENVALUES:
        for name, direction in (("along", normal), ("across", across)):
            key = free.pop()
            v = vmap.add(key, (np.array(key) + 0.5) * VOXEL - 0.1 * direction, sym(Un @ np.diag([1.0, 1.0, lam + 1e-2]) @ Un.T))
            voxels.append((v, f"normal eigenvalue {lam:g}, e {name}"))
    for replica in range(2):
        Rg = random_rotation(rng)
        g = Group(f"indefinite {replica}", "indefinite", rng.uniform(-3, 3, size=3),
                  cm(sym(Rg.T @ Un @ np.diag([1.0, 1.0, -1e-2]) @ Un.T @ Rg)))
        for angle in (0.0, 1.0, 2.5):
            R = axis_rotation(normal, angle) @ Rg
            g.cases += [_case(vmap, g.x, R, v, f"{name}, turned by {angle:g}") for v, name in voxels]
        groups.append(g)
    indefinite_voxels = voxels

    # asymmetry: c01 != c10 — twelve planes are read, S and W are not symmetric
    for delta in ASYMMETRIES:
        C = regularised()
        C[0, 1] += delta
        g = Group(f"asymmetry {delta:g}", "asymmetry", rng.uniform(-3, 3, size=3), cm(C))
        g.cases = [_case(vmap, g.x, R, scale_voxel[1.0], name) for name, R in rotations + randoms[:10]]
        groups.append(g)

    # distance and |e|: x in eighths, so that the identity pose is exact and |e| = 0 is met exactly
    for dname, keys in DISTANCES:
        x = np.zeros(3) if dname == "0" else rng.integers(-16, 17, size=3) / 8.0
        g = Group(f"distance {dname}", "distance", x, cm(regularised()))
        if dname == "0":
            v = vmap.add(keys[0], 0.1 * _unit(rng), V0)        # p = R 0 + 0 = 0 exactly, e = -mean
            g.cases = [Case(np.array(R), np.zeros(3), v, transform(R, np.zeros(3), x), f"{name}, |e| 0.1")
                       for name, R in rotations + randoms[:5]]
        else:
            for kj, size in zip(keys, RESIDUALS):
                v = vmap.add(kj, (np.array(kj) + 0.5) * VOXEL - size * _unit(rng), V0)
                g.cases += [_case(vmap, g.x, R, v, f"{name}, |e| {size:g}") for name, R in rotations + randoms[:5]]
        groups.append(g)

    # exact anchors: R = I, every product and sum of the term exact
    key_a, key_b = free.pop(), free.pop()
    diag = np.diag([0.25, 2.0, 16.0])
    va = vmap.add(key_a, np.array(key_a) + np.array([1, 7, 5]) / 8.0, diag)
    vb = vmap.add(key_b, np.array(key_b) + np.array([-3, 2, 9]) / 8.0, diag)
    g = Group("anchor: S a diagonal of powers of two", "anchor", np.array([3, 5, -1]) / 8.0, np.zeros(9), exact=True)
    for v, frac in ((va, (3, 1, 6)), (vb, (7, 5, 2))):
        target = np.array(vmap.keys[v]) + np.array(frac) / 8.0
        g.cases.append(_case(vmap, g.x, np.eye(3), v, "diagonal", target))
    groups.append(g)
    key_c, key_d = free.pop(), free.pop()
    vc = vmap.add(key_c, np.array(key_c) + np.array([2, 3, 7]) / 8.0, np.eye(3))
    vd = vmap.add(key_d, np.array(key_d) + np.array([9, -1, 4]) / 8.0, np.eye(3))
    shear = np.zeros((3, 3))
    shear[0, 1] = 1.0                                           # S = [[1, 1, 0], [0, 1, 0], [0, 0, 1]]
    g = Group("anchor: S a shear", "anchor", np.array([-2, 1, 6]) / 8.0, cm(shear), exact=True)
    for v, frac in ((vc, (5, 6, 1)), (vd, (1, 3, 4))):
        target = np.array(vmap.keys[v]) + np.array(frac) / 8.0
        g.cases.append(_case(vmap, g.x, np.eye(3), v, "shear", target))
    groups.append(g)

    # voxels of the weight groups (weight_groups below)
    extra = {"tiny": vmap.add(WEIGHT_KEY, np.zeros(3), 1e-14 * V0)}
    for name, offset in (("unit e 1", (1.0, 0.0, 0.0)), ("unit e 2", (2.0, 0.0, 0.0)), ("unit e 0", (0.0, 0.0, 0.0))):
        key = [k for k in free if k[0] == 1][0]                 # centre 1.5: its neighbour above is 1.5 + 2^-52
        free.remove(key)
        extra[name] = vmap.add(key, (np.array(key) + 0.5) * VOXEL - np.array(offset), np.eye(3))
    extra["negative"] = [v for v, name in indefinite_voxels if name == "normal eigenvalue -0.005, e along"][0]
    extra["indefinite C9"] = groups[[g.name for g in groups].index("indefinite 0")].C9
    extra["indefinite R"] = groups[[g.name for g in groups].index("indefinite 0")].cases[0].R
    extra["tiny C9"] = cm(1e-14 * regularised())
    return vmap, groups, extra


def all_cases():
    vmap, groups = sweep()
    return [(g, k, c) for g in groups for k, c in enumerate(g.cases)]


@lru_cache(maxsize=1)
def references():
    """{(group name, case index): Term} over the sweep, computed once."""
    vmap, groups = sweep()
    return {(g.name, k): term(c.R, c.p, g.C9, vmap.means[c.voxel], vmap.covs[c.voxel])
            for g in groups for k, c in enumerate(g.cases)}


# ---- the weight --------------------------------------------------------------------------------------------------------
# (kernel, c, gate): the library holds c and the gate as millionths, 1.0 / 2.0 / 4.0 exactly
SETTINGS = ((HUBER, 1.0, 0.0), (HUBER, 2.0, 0.0), (CAUCHY, 1.0, 0.0), (CAUCHY, 2.0, 0.0), (NONE, 1.0, 1.0), (NONE, 1.0, 4.0),
            (CAUCHY, 1.0, 4.0), (CAUCHY, 2.0, 1.0))
NEAR = 1e-12                 # the 20 values either side of c^2 lie within this, relative


def _multipliers():
    """d^2 / c^2 (or / gate) of the log sweep: 1e-12, 1.7 x 10^k for k = -12 .. 11, 1e12.  No value is 1 or 4 or a quarter:
    a gate is never met to within a rounding."""
    return [1e-12] + [1.7 * 10.0 ** k for k in range(-12, 12)] + [1e12]


@lru_cache(maxsize=1)
def weight_groups():
    """[Group] with .robust set: per (kernel, c, gate) the poses of ONE point (R = I) against the 1e-14-scaled voxel,
    p moved inside the voxel so that d^2 sweeps 1e-12 ... 1e12 times c^2 (times the gate for the gate alone), with 20 values
    within 1e-12 relative of c^2 on both sides where a kernel is set and c^2 is not the gate; and one group of exact cases
    per setting (S = I, e = (1, 0, 0), (1 + 2^-52, 0, 0), (2, 0, 0), 0) plus the negative raw residual of the indefinite
    class.  The reference decides count and weight; where a case is exact its bound is zero."""
    vmap, _, extra = _build()
    rng = np.random.default_rng(99)
    tiny, C9 = extra["tiny"], extra["tiny C9"]
    x = np.zeros(3)                                               # p = fl(I 0 + t) = t: e = p - 0 takes every fp64 value
    direction = -np.abs(_unit(rng))
    q = term(np.eye(3), direction, C9, np.zeros(3), vmap.covs[tiny]).raw      # d^2 = s^2 q for e = s direction
    out = []
    for kernel, c, gate in SETTINGS:
        unit = c * c if kernel != NONE else gate
        targets = [m * unit for m in _multipliers()]
        if kernel != NONE and c * c != gate:
            offsets = np.linspace(NEAR / 20, NEAR, 20)
            targets += [c * c * (1.0 + o) for o in offsets] + [c * c * (1.0 - o) for o in offsets]
        if gate > 0.0:
            targets += [gate * (1.0 + 1e-6), gate * (1.0 - 1e-6)]
        g = Group(f"weight sweep {kernel} c {c:g} gate {gate:g}", "weight", x, C9, robust=(kernel, c, gate))
        for d2 in targets:
            with mp.workdps(DPS):
                s = float(mpmath.sqrt(mpf(d2) / q))
            assert s < 0.45, (d2, s)
            g.cases.append(_case(vmap, x, np.eye(3), tiny, f"d^2 {d2!r}", s * direction))
        out.append(g)
        # exact: C = 0, C_voxel = I, R = I, p = x + t in eighths
        xe = np.array([1, -3, 2]) / 8.0
        g = Group(f"weight exact {kernel} c {c:g} gate {gate:g}", "weight", xe, np.zeros(9), exact=True, robust=(kernel, c, gate))
        for name in ("unit e 1", "unit e 2", "unit e 0"):
            g.cases.append(_case(vmap, xe, np.eye(3), extra[name], name))
        above = vmap.centre(extra["unit e 1"]).copy()
        above[0] = np.nextafter(above[0], np.inf)
        g.cases.append(_case(vmap, xe, np.eye(3), extra["unit e 1"], "unit e 1 + 2^-52", above))
        out.append(g)
        # a negative raw residual: d^2 is 0, the weight is 1 and the gate is passed
        xi = rng.uniform(-3, 3, size=3)
        g = Group(f"weight negative raw {kernel} c {c:g} gate {gate:g}", "weight", xi, extra["indefinite C9"], robust=(kernel, c, gate))
        g.cases.append(_case(vmap, xi, extra["indefinite R"], extra["negative"], "negative raw residual"))
        out.append(g)
    return out
