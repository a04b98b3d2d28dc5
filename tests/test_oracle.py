"""Pins the CPU oracle (the checker of every GPU parity test) — runs without a GPU.

The reference has no tests, golden vectors or fixtures for this path and cannot be
built here, so the oracle is pinned by (1) analytic known-answer tests K1-K6,
(2) an independently written numpy restatement, (3) committed golden outputs (regression).
PARITY UNPINNED by the reference's own tests.
"""
import os

import numpy as np
import pytest

from conftest import pose_error
from eskf_lio_amd import synth
from oracle import vgicp_numpy as npo

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def skew(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0.0]])


# ---- K1: one correspondence, Sigma = I ------------------------------------------------------
def test_k1_single_residual_blocks(oracle):
    p = np.array([1.0, 2.0, 3.0])
    e = np.array([0.1, -0.2, 0.05])
    JTJ, JTr = oracle.jtj_jtr(p, p - e, np.eye(3))      # r = p - mu = e
    J = np.hstack([np.eye(3), -skew(p)])                # [I | -[p]x], state [translation; rotation]
    assert np.allclose(JTJ, J.T @ J, rtol=0, atol=1e-14)
    assert np.allclose(JTr, J.T @ e, rtol=0, atol=1e-14)
    # written out by hand for p = (1,2,3):
    assert JTJ[0, 4] == 3.0 and JTJ[0, 5] == -2.0 and JTJ[1, 3] == -3.0 and JTJ[2, 4] == -1.0
    assert JTJ[3, 3] == 13.0 and JTJ[4, 4] == 10.0 and JTJ[5, 5] == 5.0 and JTJ[3, 4] == -2.0


def test_k1_general_covariance_matches_dense_formula(oracle):
    rng = np.random.default_rng(1)
    for _ in range(20):
        p, mu = rng.normal(size=3) * 5, rng.normal(size=3) * 5
        A = rng.normal(size=(3, 3))
        cov = A @ A.T + 0.1 * np.eye(3)
        JTJ, JTr = oracle.jtj_jtr(p, mu, cov)
        J = np.hstack([np.eye(3), -skew(p)])
        W = np.linalg.inv(cov)
        assert np.allclose(JTJ, J.T @ W @ J, rtol=1e-11, atol=1e-11)
        assert np.allclose(JTr, J.T @ W @ (p - mu), rtol=1e-11, atol=1e-11)


# ---- K2: exact structured scan recovers the motion ------------------------------------------
def test_k11_one_round_in_exact_rational_arithmetic(oracle):
    """A pin that shares no floating-point code with the oracle or the numpy restatement: one round of the
    path on a handful of correspondences evaluated with exact rationals (fractions.Fraction) — transform of the
    point and R C R^T (Open3D), Sigma = R C R^T + C_voxel, its inverse by cofactors, J = [I | -[p]x],
    J^T Sigma^-1 J and J^T Sigma^-1 (p - mu), summed (src/Registration.cpp:52-102) — on inputs that are exactly
    representable, so the exact result is THE result and the oracle must reproduce it to rounding."""
    from fractions import Fraction as Fr
    rng = np.random.default_rng(11)
    h = 0.5
    n = 6
    # a rotation with rational entries (Cayley transform of a small skew matrix), exact in Fractions; points,
    # means and covariances on a dyadic grid
    a, b, c = Fr(1, 8), Fr(-1, 16), Fr(3, 32)
    A = [[Fr(0), -c, b], [c, Fr(0), -a], [-b, a, Fr(0)]]
    eye = [[Fr(int(i == j)) for j in range(3)] for i in range(3)]

    def mat(f):
        return [[f(i, j) for j in range(3)] for i in range(3)]

    def mul(X, Y):
        return mat(lambda i, j: sum(X[i][k] * Y[k][j] for k in range(3)))

    def inv(M):
        cof = mat(lambda i, j: M[(i + 1) % 3][(j + 1) % 3] * M[(i + 2) % 3][(j + 2) % 3]
                  - M[(i + 1) % 3][(j + 2) % 3] * M[(i + 2) % 3][(j + 1) % 3])
        det = sum(M[0][j] * cof[0][j] for j in range(3))
        return mat(lambda i, j: cof[j][i] / det)

    R = mul(inv(mat(lambda i, j: eye[i][j] - A[i][j])), mat(lambda i, j: eye[i][j] + A[i][j]))   # (I - A)^-1 (I + A)
    t = [Fr(1, 4), Fr(-1, 8), Fr(1, 16)]
    Rf = np.array([[float(x) for x in row] for row in R])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rf, [float(x) for x in t]
    # the float rotation is not the exact rational one; rebuild the exact inputs FROM the floats the oracle gets
    Rq = [[Fr(float(Rf[i, j])) for j in range(3)] for i in range(3)]
    cells = rng.integers(-4, 5, size=(n, 3))
    means = (cells + rng.integers(1, 8, size=(n, 3)) / 8.0) * h
    pts_map = (cells + rng.integers(1, 8, size=(n, 3)) / 8.0) * h                   # where the points must land
    def dyadic_spd():
        L = np.tril(rng.integers(-3, 4, size=(3, 3)) / 4.0) + np.eye(3)
        return L @ L.T
    cov_v = np.array([dyadic_spd() for _ in range(n)])
    cov_s = np.array([dyadic_spd() for _ in range(n)])
    # source points: exact pre-images are not representable in general, so choose scan points on a dyadic grid
    # and let the EXACT arithmetic tell where they land and whether they still hit the intended voxel
    pts = rng.integers(-40, 41, size=(n, 3)) / 16.0
    JTJ_x = [[Fr(0)] * 6 for _ in range(6)]
    JTr_x = [Fr(0)] * 6
    keep_means, count = [], 0
    om = oracle.OracleMap(h, 1)
    used = set()
    for i in range(n):
        p = [Fr(float(v)) for v in pts[i]]
        q = [sum(Rq[r][k] * p[k] for k in range(3)) + Fr(float(T[r, 3])) for r in range(3)]
        key = tuple(int(np.floor(float(qq) / h)) for qq in q)
        if key in used:
            continue
        used.add(key)
        mu = [(Fr(key[r]) + Fr(int(rng.integers(1, 8)), 8)) * Fr(h) for r in range(3)]   # a voxel mean inside that voxel
        keep_means.append(([float(m) for m in mu], cov_v[i].T.reshape(9)))
        C = [[Fr(float(cov_s[i][r][k])) for k in range(3)] for r in range(3)]
        Cv = [[Fr(float(cov_v[i][r][k])) for k in range(3)] for r in range(3)]
        Rt = mat(lambda r, k: Rq[k][r])
        S = mul(mul(Rq, C), Rt)
        S = mat(lambda r, k: S[r][k] + Cv[r][k])
        W = inv(S)
        J = [[Fr(int(r == k)) for k in range(3)] + [Fr(0)] * 3 for r in range(3)]
        J[0][4], J[0][5] = q[2], -q[1]                                   # -[q]x
        J[1][3], J[1][5] = -q[2], q[0]
        J[2][3], J[2][4] = q[1], -q[0]
        e = [q[r] - mu[r] for r in range(3)]
        JT_W = [[sum(J[k][r] * W[k][cidx] for k in range(3)) for cidx in range(3)] for r in range(6)]
        for r in range(6):
            JTr_x[r] += sum(JT_W[r][k] * e[k] for k in range(3))
            for cc in range(6):
                JTJ_x[r][cc] += sum(JT_W[r][k] * J[k][cc] for k in range(3))
        count += 1
    om.insert(np.array([m for m, _ in keep_means]), np.array([cv for _, cv in keep_means]))
    tp, tc = oracle.transform(pts, cov_s.transpose(0, 2, 1).reshape(n, 9), T)
    JTJ, JTr, m = om.accumulate(tp, tc)
    assert m == count >= 4
    exact_J = np.array([[float(x) for x in row] for row in JTJ_x])
    exact_r = np.array([float(x) for x in JTr_x])
    assert np.allclose(JTJ, exact_J, rtol=1e-12, atol=1e-12 * np.abs(exact_J).max())
    assert np.allclose(JTr, exact_r, rtol=1e-11, atol=1e-12 * np.abs(exact_J).max())


def test_k2_noise_free_structured_scan_recovers_pose(oracle):
    vmap = synth.make_map(4_000, seed=11)
    pts, covs, T_true = synth.make_structured_scan(1_500, vmap, seed=12, noise=0.0)
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    r = om.align(pts, covs, np.eye(4), 50, 1e-12, 1.0 - 1e-12)
    dt, dr = pose_error(r.pose, T_true)
    assert dt < 1e-9 and dr < 1e-9
    assert r.corr_count[-1] == 1_500                       # every point lands in its own voxel
    # one Gauss-Newton step from identity is already O(|phi|^2) close
    one = om.align(pts, covs, np.eye(4), 1, 1e-12, 2.0)
    dt1, dr1 = pose_error(one.pose, T_true)
    assert dt1 < 5e-3 and dr1 < 5e-4


# ---- K3: no correspondences -----------------------------------------------------------------
def test_k3_zero_matches_returns_guess_and_converges(oracle):
    vmap = synth.make_map(500, seed=3)
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    pts, covs = synth.make_uniform_scan(64, vmap, seed=4)
    far = pts + 1.0e4                                      # entirely outside the map
    g = synth.default_guess()
    r = om.align(far, covs, g, 10, 1e-6, 0.9999)
    assert r.iterations == 1 and r.converged and r.corr_count[0] == 0
    assert np.array_equal(r.pose, g)                       # zero system -> zero step -> pose = guess
    empty = oracle.OracleMap(0.3, 1)
    r = empty.align(pts, covs, g, 10, 1e-6, 0.9999)
    assert r.iterations == 1 and r.converged and np.array_equal(r.pose, g)
    se3, step = oracle.solve_step(np.zeros((6, 6)), np.zeros(6))
    assert not se3.any() and np.array_equal(step, np.eye(4))


# ---- K4: se3ToSE3 -----------------------------------------------------------------------------
def test_k4_se3_exponential(oracle):
    assert np.array_equal(oracle.se3_to_SE3(np.zeros(6)), np.eye(4))
    T = oracle.se3_to_SE3([1.0, 2.0, 3.0, 0.0, 0.0, 0.0])
    assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], [1.0, 2.0, 3.0])
    # below the 1e-6 branch: J = I exactly, R is still a proper small rotation
    T = oracle.se3_to_SE3([1.0, 2.0, 3.0, 1e-7, 0.0, 0.0])
    assert np.array_equal(T[:3, 3], [1.0, 2.0, 3.0])
    assert abs(T[2, 1] - 1e-7) < 1e-20 and abs(T[1, 2] + 1e-7) < 1e-20
    # 90 degrees about z
    T = oracle.se3_to_SE3([0.0, 0.0, 0.0, 0.0, 0.0, np.pi / 2])
    assert np.allclose(T[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    # general: against the independent numpy restatement and scipy
    from scipy.spatial.transform import Rotation
    xi = np.array([0.3, -0.2, 0.5, 0.4, -0.7, 0.2])
    T = oracle.se3_to_SE3(xi)
    assert np.allclose(T[:3, :3], Rotation.from_rotvec(xi[3:]).as_matrix(), atol=1e-15)
    assert np.allclose(T, npo.se3_to_SE3(xi), atol=1e-15)
    assert np.allclose(T, synth.se3_to_SE3(xi), atol=1e-15)


# ---- K5: convergence thresholds are non-strict on the converged side -----------------------
def test_k5_convergence_check_boundaries(oracle):
    step = np.eye(4)
    step[:3, 3] = [1e-3, 0.0, 0.0]                         # |t|^2 == 1e-6 exactly? (1e-3)^2 rounds
    tsq = float(step[0, 3] ** 2)
    assert oracle.convergence_check(step, 1.0, tsq)        # equality counts as converged
    assert not oracle.convergence_check(step, 1.0, np.nextafter(tsq, 0.0))
    R = oracle.se3_to_SE3([0, 0, 0, 0, 0, 0.01])
    cosine = 0.5 * (np.trace(R[:3, :3]) - 1.0)
    assert oracle.convergence_check(R, cosine, 1.0)
    assert not oracle.convergence_check(R, np.nextafter(cosine, 2.0), 1.0)
    assert not oracle.convergence_check(np.eye(4), 2.0, 1.0)   # cosine_threshold > 1 never converges


# ---- K6: voxel keys: floor of a true division ------------------------------------------------
def test_k6_voxel_index_floor_semantics(oracle):
    pts = np.array([[-0.1, 0.0, 0.3], [-0.3, 0.29999999999999993, 0.6], [-0.30000000000000004, 0.9, -1e-300],
                    [1e-300, -0.0, 299.99999999999994]])
    keys = oracle.voxel_index(0.3, pts)
    expect = np.floor(pts / 0.3).astype(np.int32)
    assert np.array_equal(keys, expect)
    assert keys[0].tolist() == [-1, 0, 1]                  # floor, not truncation
    assert keys[1].tolist() == [-1, 0, 2] and keys[2].tolist() == [-2, 3, -1]
    rng = np.random.default_rng(5)
    rnd = rng.uniform(-50, 50, size=(20000, 3))
    on_face = np.round(rnd / 0.3) * 0.3                    # exact multiples of the voxel size
    for p in (rnd, on_face):
        assert np.array_equal(oracle.voxel_index(0.3, p), np.floor(p / 0.3).astype(np.int32))


# ---- voxel statistics: the reference's running-mean insertion rule ---------------------------
def test_map_insertion_rule(oracle):
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1.0, 1.0, size=(400, 3))
    A = rng.normal(size=(400, 3, 3))
    covs = (A @ A.transpose(0, 2, 1)).transpose(0, 2, 1).reshape(400, 9)
    for cap in (1, 3, 1000):
        om = oracle.OracleMap(0.3, cap)
        om.insert(pts, covs)
        nm = npo.NumpyMap(0.3, cap)
        nm.insert(pts, covs)
        keys, means, mcovs, counts = om.export()
        assert len(om) == len(nm) == len({tuple(k) for k in np.floor(pts / 0.3).astype(int)})
        for k, m, c, n in zip(map(tuple, keys), means, mcovs, counts):
            cnt, mean, cov = nm._dict[k]
            assert n == cnt and n <= cap
            assert np.allclose(m, mean, atol=1e-15) and np.allclose(c.reshape(3, 3).T, cov, atol=1e-14)
    # cap = 1 freezes the first point of each voxel
    om = oracle.OracleMap(0.3, 1)
    om.insert(pts, covs)
    keys, means, _, counts = om.export()
    first = {}
    for p, k in zip(pts, map(tuple, np.floor(pts / 0.3).astype(int))):
        first.setdefault(k, p)
    assert all(np.array_equal(first[tuple(k)], m) for k, m in zip(keys, means)) and (counts == 1).all()


# ---- open3d Transform semantics ---------------------------------------------------------------
def test_transform_semantics(oracle):
    rng = np.random.default_rng(9)
    pts = rng.normal(size=(50, 3))
    A = rng.normal(size=(50, 3, 3))
    C = A @ A.transpose(0, 2, 1)
    T = synth.se3_to_SE3([0.5, -1.0, 2.0, 0.3, 0.2, -0.4])
    tp, tc = oracle.transform(pts, C.transpose(0, 2, 1).reshape(50, 9), T)
    assert np.allclose(tp, pts @ T[:3, :3].T + T[:3, 3], atol=1e-14)
    assert np.allclose(tc.reshape(50, 3, 3).transpose(0, 2, 1), T[:3, :3] @ C @ T[:3, :3].T, atol=1e-13)


# ---- cross-implementation: C++ oracle vs numpy restatement ------------------------------------
def test_oracle_matches_numpy_restatement_c1(oracle, c1_inputs, c1_oracle_map):
    vmap, pts, covs = c1_inputs
    nm = npo.NumpyMap(vmap.voxel_size, 1)
    nm.insert(vmap.means, vmap.covs)
    g = synth.default_guess()
    r = c1_oracle_map.align(pts, covs, g, 20, 1e-6, 2.0)
    T, counts, JTJs, JTrs, conv = npo.align(nm, pts, covs, g, 20, 1e-6, 2.0)
    assert r.iterations == 20 and not r.converged and not conv
    assert np.array_equal(counts, r.corr_count)
    assert np.abs(T - r.pose).max() < 1e-12
    scale = np.abs(r.JTJ).max(axis=(1, 2), keepdims=True)
    assert (np.abs(JTJs - r.JTJ) <= 1e-9 * scale).all()
    assert np.abs(JTrs - r.JTr).max() <= 1e-9 * np.abs(r.JTr).max()
    # hit rate ~ occupancy 0.5, loop does not converge within 20 rounds
    assert 0.45 < r.corr_count.mean() / 5000 < 0.55


def test_oracle_matches_numpy_restatement_structured(oracle, c1_inputs, c1_oracle_map):
    vmap, _, _ = c1_inputs
    pts, covs, T_true = synth.make_structured_scan(5_000, vmap)
    nm = npo.NumpyMap(vmap.voxel_size, 1)
    nm.insert(vmap.means, vmap.covs)
    r = c1_oracle_map.align(pts, covs, np.eye(4), 100, 1e-6, 0.9999)
    T, counts, _, _, conv = npo.align(nm, pts, covs, np.eye(4), 100, 1e-6, 0.9999)
    assert r.converged and conv and r.iterations == len(counts) == 3
    assert np.array_equal(counts, r.corr_count) and r.corr_count[-1] == 5000
    assert np.abs(T - r.pose).max() < 1e-12
    dt, dr = pose_error(r.pose, T_true)
    assert dt < 2e-3 and dr < 1e-3                         # noise 1 cm / sqrt(N)


def test_faithful_mode_equals_deterministic_mode(oracle, c1_inputs, c1_oracle_map):
    """The reference-structured OpenMP mode differs only by summation order."""
    _, pts, covs = c1_inputs
    g = synth.default_guess()
    d = c1_oracle_map.align(pts, covs, g, 20, 1e-6, 2.0)
    f = c1_oracle_map.align(pts, covs, g, 20, 1e-6, 2.0, mode=oracle.FAITHFUL)
    assert np.array_equal(d.corr_count, f.corr_count)
    assert np.abs(d.pose - f.pose).max() < 1e-12


def test_point_order_does_not_matter(oracle, c1_inputs, c1_oracle_map):
    _, pts, covs = c1_inputs
    g = synth.default_guess()
    perm = np.random.default_rng(3).permutation(pts.shape[0])
    a = c1_oracle_map.align(pts, covs, g, 20, 1e-6, 2.0)
    b = c1_oracle_map.align(pts[perm], covs[perm], g, 20, 1e-6, 2.0)
    assert np.array_equal(a.corr_count, b.corr_count) and np.abs(a.pose - b.pose).max() < 1e-12


# ---- golden fixtures ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_uniform", "c1_structured"])
def test_golden_regression(oracle, c1_inputs, c1_oracle_map, name):
    vmap, pts, covs = c1_inputs
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    if name == "c1_structured":
        pts, covs, _ = synth.make_structured_scan(5_000, vmap)
    max_it, tsq, cos = g["params"]
    r = c1_oracle_map.align(pts, covs, g["guess"], int(max_it), tsq, cos)
    assert r.iterations == int(g["iterations"]) and r.converged == bool(g["converged"])
    assert np.array_equal(r.corr_count, g["corr_count"])
    assert np.abs(r.pose - g["pose"]).max() < 1e-13
    assert np.allclose(r.JTJ, g["JTJ"], rtol=1e-12, atol=0)


def test_golden_tiny_is_hermetic(oracle):
    g = np.load(os.path.join(GOLDEN, "tiny.npz"))
    om = oracle.OracleMap(float(g["voxel_size"]), 1)
    om.insert(g["means"], g["covs"])
    max_it, tsq, cos = g["params"]
    r = om.align(g["points"], g["point_covs"], g["guess"], int(max_it), tsq, cos)
    assert np.array_equal(r.corr_count, g["corr_count"]) and np.abs(r.pose - g["pose"]).max() < 1e-13
    nm = npo.NumpyMap(float(g["voxel_size"]), 1)
    nm.insert(g["means"], g["covs"])
    T, counts, *_ = npo.align(nm, g["points"], g["point_covs"], g["guess"], int(max_it), tsq, cos)
    assert np.array_equal(counts, g["corr_count"]) and np.abs(T - g["pose"]).max() < 1e-11


def test_synthetic_inputs_are_reproducible(c1_inputs):
    """Seeds regenerate the exact bits the fixtures were made from (IEEE-exact generator)."""
    import hashlib
    vmap, pts, covs = c1_inputs
    g = np.load(os.path.join(GOLDEN, "c1_uniform.npz"))
    h = hashlib.sha256()
    for a in (vmap.keys, vmap.means, vmap.covs, pts, covs):
        h.update(np.ascontiguousarray(a).tobytes())
    assert np.frombuffer(h.digest()[:8], dtype=np.uint64)[0] == g["input_checksum"]
    assert vmap.side == 47 and vmap.keys.shape == (50_000, 3)
    assert len({tuple(k) for k in vmap.keys}) == 50_000
    assert np.array_equal(np.floor(vmap.means / 0.3).astype(np.int32), vmap.keys)
    C = covs.reshape(-1, 3, 3)
    assert np.array_equal(C, C.transpose(0, 2, 1))
    ev = np.linalg.eigvalsh(C[:100])
    assert np.allclose(ev, [0.01, 1.0, 1.0], atol=1e-12)   # R diag(1,1,1e-2) R^T


# ---- scan preparation: oracle vs the numpy restatement -------------------------
def _cov_mats(c9):
    return np.asarray(c9).reshape(-1, 3, 3).transpose(0, 2, 1)


def test_preprocess_oracle_matches_numpy(oracle):
    """First point per voxel, 30 nearest neighbours, cumulant covariance, U diag(1,1,1e-2) V^T
    (CloudPreprocessor.cpp:76-127): Eigen's JacobiSVD restated in the oracle, LAPACK's SVD in numpy."""
    pts = synth.make_lidar_scan(3_000)
    op, oc, ix = oracle.preprocess(pts, 0.3, 30)
    npts, ncov, nix = npo.preprocess(pts, 0.3, 30)
    assert np.array_equal(ix, nix.astype(np.uint64)) and np.array_equal(op, npts)
    assert 0 < len(ix) < 3_000 and np.all(np.diff(ix.astype(np.int64)) > 0)
    assert np.abs(_cov_mats(oc) - ncov).max() < 1e-10
    # every covariance is I - 0.99 u3 u3^T for a unit u3: eigenvalues (1e-2, 1, 1)
    ev = np.linalg.eigvalsh(_cov_mats(oc))
    assert np.allclose(ev, [1e-2, 1.0, 1.0], atol=1e-12)


def test_preprocess_known_answers(oracle):
    # K7: points on the plane z = 0 -> normal is z: covariance diag(1, 1, 1e-2)
    g = np.arange(8, dtype=np.float64)
    plane = np.stack([*np.meshgrid(g * 0.11, g * 0.13, indexing="ij"), np.zeros((8, 8))], axis=-1).reshape(-1, 3)
    _, oc, ix = oracle.preprocess(plane, 0.3, 30)
    assert np.allclose(_cov_mats(oc), np.diag([1.0, 1.0, 1e-2]), atol=1e-12)
    # the kept point of a voxel is its first point in scan order
    keys = np.floor(plane / 0.3).astype(np.int32)
    first = {}
    for i, k in enumerate(map(tuple, keys)):
        first.setdefault(k, i)
    assert sorted(first.values()) == list(ix.astype(np.int64))
    # K8: fewer than three neighbours available -> identity before the regularisation
    _, oc, ix = oracle.preprocess(np.array([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0]]), 0.3, 30)
    assert len(ix) == 2 and np.allclose(_cov_mats(oc), np.diag([1.0, 1.0, 1e-2]), atol=1e-15)
    # empty scan
    assert len(oracle.preprocess(np.zeros((0, 3)), 0.3, 30)[2]) == 0


def test_jacobi_svd_restatement_against_lapack(oracle):
    """The oracle's Eigen::JacobiSVD<Matrix3d> restatement (published operation order) on ANY real 3x3 -- general,
    symmetric, rank-deficient, scaled over ten decades -- against LAPACK: reconstruction, orthogonality, singular
    values, descending order.  This is the independent pin of the regulariser's arithmetic
    (src/CloudPreprocessor.cpp:119-123)."""
    rng = np.random.default_rng(11)
    for k in range(3000):
        A = rng.standard_normal((3, 3)) * 10.0 ** rng.uniform(-5, 5)
        if k % 3 == 0:
            A = A + A.T
        if k % 7 == 0:
            A[:, 2] = 2.0 * A[:, 0]
        U, sv, V, _ = oracle.jacobi_svd3(A)
        scale = np.abs(A).max()
        assert np.abs(U @ np.diag(sv) @ V.T - A).max() <= 2e-14 * scale
        assert np.abs(U.T @ U - np.eye(3)).max() <= 2e-14 and np.abs(V.T @ V - np.eye(3)).max() <= 2e-14
        assert sv[0] >= sv[1] >= sv[2] >= 0.0
        assert np.abs(sv - np.linalg.svd(A, compute_uv=False)).max() <= 2e-14 * scale
    # exact cases: the zero matrix and the identity need no rotation: U = V = I, F comes out as it is
    for A in (np.zeros((3, 3)), np.eye(3), np.diag([3.0, 2.0, 1.0])):
        R, neg = oracle.regularize(A)
        assert neg == 0 and np.array_equal(R, np.diag([1.0, 1.0, 1e-2]))
    # values in ascending order on the diagonal: the sort moves the columns, the small factor follows the small value
    R, _ = oracle.regularize(np.diag([1.0, 2.0, 3.0]))
    assert np.array_equal(R, np.diag([1e-2, 1.0, 1.0]))
    assert oracle.jacobi_svd3(np.full((3, 3), np.nan))[3] == -1


def test_regulariser_carries_the_sign_of_a_negative_eigenvalue(oracle):
    """U F V^T of a symmetric matrix is sum_k f_k sign(lambda_k) q_k q_k^T ordered by |lambda| (an SVD has S >= 0,
    so the sign of a negative eigenvalue sits in U against V): what the reference's JacobiSVD line does, checked
    against LAPACK's SVD and against the closed form."""
    rng = np.random.default_rng(5)
    F = np.diag([1.0, 1.0, 1e-2])
    for _ in range(2000):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        lam = rng.standard_normal(3) * 10.0 ** rng.uniform(-3, 3, 3)
        a = np.sort(np.abs(lam))
        if a[1] < 1.01 * a[0] or a[2] < 1.01 * a[1]:
            continue                                   # (near-)equal |lambda|: which direction gets 1e-2 is not defined
        A = Q @ np.diag(lam) @ Q.T
        A = 0.5 * (A + A.T)
        R, neg = oracle.regularize(A)
        assert neg == int((lam < 0).sum())
        order = np.argsort(-np.abs(lam))
        want = sum(f * np.sign(lam[k]) * np.outer(Q[:, k], Q[:, k]) for f, k in zip((1.0, 1.0, 1e-2), order))
        tol = 1e-12 * a[2] / min(a[1] - a[0], a[2] - a[1])           # directions are as good as the gaps allow
        assert np.abs(R - want).max() < tol
        Us, _, Vt = np.linalg.svd(A)
        assert np.abs(R - Us @ F @ Vt).max() < tol


def _degenerate_scans():
    """Neighbourhoods whose cumulant covariance E[xx^T] - E[x]E[x]^T has rounding-level eigenvalues far from the
    origin: an exact tilted plane, collinear points, repeated points."""
    rng = np.random.default_rng(3)
    n = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    b1 = np.cross(n, [1.0, 0.0, 0.0])
    b1 /= np.linalg.norm(b1)
    b2 = np.cross(n, b1)
    uv = rng.uniform(-1.5, 1.5, (600, 2))
    plane = np.array([50.0, -70.0, 40.0]) + uv[:, :1] * b1 + uv[:, 1:] * b2
    line = np.array([-30.0, 20.0, 60.0]) + rng.uniform(-2.0, 2.0, (200, 1)) * np.array([2.0, -1.0, 0.5]) / np.sqrt(5.25)
    same = np.repeat(np.array([[80.3, -41.7, 12.9]]), 40, axis=0)
    return plane, n, line, same


def test_preprocess_degenerate_neighbourhoods(oracle):
    """KATs for the behaviour class VERDICT r2 reproduced: the reference can emit an INDEFINITE covariance. Exact plane:
    eigenvalues (+-1e-2, 1, 1), the +-1e-2 direction is the plane's normal, the count of indefinite points is
    reported; numpy (LAPACK SVD) agrees up to the sign of the rounding-level term, which no restatement can pin."""
    plane, normal, line, same = _degenerate_scans()
    op, oc, ix, bad = oracle.preprocess_ex(plane, 0.3, 30)
    C = _cov_mats(oc)
    ev, evec = np.linalg.eigh(C)
    small = np.argmin(np.abs(ev), axis=1)
    assert np.allclose(np.sort(np.abs(ev), axis=1), [1e-2, 1.0, 1.0], atol=1e-9)
    nrm = evec[np.arange(len(C)), :, small]
    assert np.all(np.abs(np.abs(nrm @ normal) - 1.0) < 1e-6)
    negative = int((ev[np.arange(len(C)), small] < 0).sum())
    assert bad == negative                                            # the count the caller can see
    assert 0 < negative < len(C)                                      # this input does reach the indefinite class
    _, ncov, nix = npo.preprocess(plane, 0.3, 30)
    assert np.array_equal(ix, nix.astype(np.uint64))
    flip = 0.02 * nrm[:, :, None] * nrm[:, None, :]                   # the +-1e-2 n n^T term, either sign
    d = np.abs(C - ncov).reshape(len(C), -1).max(axis=1)
    d_flipped = np.minimum(np.abs(C + flip - ncov).reshape(len(C), -1).max(axis=1),
                           np.abs(C - flip - ncov).reshape(len(C), -1).max(axis=1))
    assert np.all(np.minimum(d, d_flipped) < 1e-6)
    # collinear points: one direction carries the variance, the other two eigenvalues are BOTH noise (either sign, nearly
    # equal in size, so U and V may even disagree inside that plane and the result need not be symmetric): what is
    # defined is that the singular values of U F V^T are (1, 1, 1e-2) and that the line's direction keeps the factor 1
    _, oc, _, _ = oracle.preprocess_ex(line, 0.3, 30)
    C = _cov_mats(oc)
    assert np.allclose(np.linalg.svd(C, compute_uv=False), [1.0, 1.0, 1e-2], atol=1e-9)
    along = np.array([2.0, -1.0, 0.5]) / np.sqrt(5.25)
    assert np.allclose(np.einsum("i,nij,j->n", along, C, along), 1.0, atol=1e-6)
    # K identical points: every eigenvalue is noise (sum of 30 equal terms / 30 is not the term): singular values only
    _, oc, ix, _ = oracle.preprocess_ex(same, 0.3, 30)
    assert len(ix) == 1 and np.allclose(np.linalg.svd(_cov_mats(oc)[0], compute_uv=False), [1.0, 1.0, 1e-2], atol=1e-9)
    # ... unless the cumulants are exact (dyadic coordinates): covariance exactly zero -> no rotation, U = V = I, F itself
    exact = np.repeat(np.array([[80.25, -41.5, 12.75]]), 40, axis=0)
    _, oc, ix, bad = oracle.preprocess_ex(exact, 0.3, 30)
    assert len(ix) == 1 and bad == 0 and np.array_equal(_cov_mats(oc)[0], np.diag([1.0, 1.0, 1e-2]))


def _restated_query_covariances(pts, query, knn):
    """oracle_preprocess's covariance of the kept points `query`, restated: the K smallest (distance², index) pairs by a
    lexicographic sort, the cumulants summed in that order, then the oracle's regulariser on the result."""
    K = min(knn, len(pts))
    out = np.zeros((len(query), 9))
    for o, q in enumerate(query):
        d = pts - pts[q]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        nb = pts[np.lexsort((np.arange(len(pts)), d2))[:K]]
        C = np.eye(3)
        if K >= 3:
            c = np.zeros(9)
            for p in nb:                                                  # one term at a time, as the reference adds them
                c += [p[0], p[1], p[2], p[0] * p[0], p[0] * p[1], p[0] * p[2], p[1] * p[1], p[1] * p[2], p[2] * p[2]]
            c /= K
            C = np.array([[c[3] - c[0] * c[0], c[4] - c[0] * c[1], c[5] - c[0] * c[2]],
                          [c[4] - c[0] * c[1], c[6] - c[1] * c[1], c[7] - c[1] * c[2]],
                          [c[5] - c[0] * c[2], c[7] - c[1] * c[2], c[8] - c[2] * c[2]]])
        out[o] = _regularized(C)
    return out


def _regularized(C):
    from oracle import binding
    return binding.regularize(C)[0].T.reshape(9)                         # column-major, as out_covs


def test_preprocess_queries_equal_the_whole_preparation(oracle):
    """oracle_preprocess_queries (the sampled checker of scans too large for the brute-force entry) gives every kept
    point's covariance of oracle_preprocess bit for bit, in any query order and with repeats; its bounded top-K keeps the
    pairs a lexicographic sort of (distance², index) keeps: a lattice where every distance occurs many times (the K-th
    place is decided by the index), a pile of exact duplicates (all at distance zero), and a LiDAR-like scan."""
    rng = np.random.default_rng(29)
    g = np.arange(-6, 7) * 0.125
    lattice = np.stack(np.meshgrid(g, g, g[:4], indexing="ij"), axis=-1).reshape(-1, 3)    # exact in binary
    lattice = np.ascontiguousarray(lattice[rng.permutation(len(lattice))])
    pile = np.concatenate([np.tile([[0.51, -0.23, 0.07]], (90, 1)), np.tile([[0.52, -0.23, 0.07]], (45, 1)),
                           rng.normal(size=(200, 3)) * 0.4, np.tile([[3.0, 3.0, 3.0]], (2, 1))])
    pile = np.ascontiguousarray(pile[rng.permutation(len(pile))])
    scan = synth.make_lidar_scan(4_000, seed=31)
    for name, pts, knn in (("lattice", lattice, 30), ("lattice", lattice, 7), ("pile", pile, 30), ("scan", scan, 30),
                           ("few", scan[:2], 30)):
        _, oc, ix = oracle.preprocess(pts, 0.3, knn)
        got = oracle.preprocess_queries(pts, 0.3, knn, ix)
        assert np.array_equal(got, oc), (name, knn)
        shuffled = rng.permutation(len(ix))
        again = np.concatenate([shuffled, shuffled[:5]])
        assert np.array_equal(oracle.preprocess_queries(pts, 0.3, knn, ix[again]), oc[again]), (name, knn)
        some = np.unique(np.concatenate([np.arange(min(40, len(ix))), rng.choice(len(ix), min(40, len(ix)), replace=False)]))
        assert np.array_equal(_restated_query_covariances(pts, ix[some].astype(np.int64), knn), oc[some]), (name, knn)
    assert oracle.preprocess_queries(scan, 0.3, 30, np.zeros(0, dtype=np.uint64)).shape == (0, 9)
    with pytest.raises(IndexError):
        oracle.preprocess_queries(scan, 0.3, 30, [len(scan)])


# ---- deskew: oracle vs the numpy restatement ------------------------------------
def _deskew_case(n=5_000, states=48, jitter=0.0, seed=9):
    st = synth.make_imu_states(states, seed=seed)
    # the sweep starts a little after the first state and ends between the last two states but one
    t = synth.make_point_times(n, st[1, 0] + 1e-4, st[-3, 0] + 0.4 / 400.0, seed=seed, jitter=jitter)
    pts = synth.make_lidar_scan(n, seed=seed)
    return pts, t, st


def test_deskew_oracle_matches_numpy(oracle):
    for jitter in (0.0, 2e-3):
        pts, t, st = _deskew_case(jitter=jitter)
        op, done = oracle.deskew(pts, t, st)
        npts, ndone = npo.deskew(pts, t, st)
        assert done == ndone and 0 < done < len(pts)
        assert np.abs(op - npts).max() < 1e-11
        assert np.array_equal(op[done:], pts[done:])               # the tail of the sweep is left as it is
        assert np.abs(op[:done] - pts[:done]).max() > 1e-3          # and the rest really moved


def test_deskew_known_answers(oracle):
    pts, t, st = _deskew_case(n=400, states=12)
    # K9: a sensor at rest: every pose equals the end pose, nothing moves (up to rounding of R^T R)
    rest = st.copy()
    rest[:, 1:4] = [1.0, -2.0, 0.5]
    rest[:, 4:] = [0.0, 0.0, np.sin(0.2), np.cos(0.2)]
    op, done = oracle.deskew(pts, t, rest)
    assert done > 0 and np.abs(op - pts).max() < 1e-13
    # K10: pure translation along x at 2 m/s: a point taken dt before the end moves by about -2 dt in x...
    lin = st.copy()
    lin[:, 1:4] = np.stack([2.0 * (st[:, 0] - st[0, 0]), 0 * st[:, 0], 0 * st[:, 0]], axis=1)
    lin[:, 4:] = [0.0, 0.0, 0.0, 1.0]
    op, done = oracle.deskew(pts, t, lin)
    shift = op[:done] - pts[:done]
    assert np.abs(shift[:, 1:]).max() == 0.0
    # ...where the pose used is the one of the first state at or after the point's time (IMU period 2.5 ms)
    state_of = np.searchsorted(lin[:, 0], t[:done], side="right")
    expect = lin[state_of, 1] - 2.0 * (t[-1] - st[0, 0])
    assert np.abs(shift[:, 0] - expect).max() < 1e-4
    # the state queue does not bracket the end of the sweep: the reference would run off it
    assert oracle.deskew(pts, t, st[:3])[1] == -1                   # no state after the last point
    assert oracle.deskew(pts, t - 1.0, st)[1] == -1                 # no state at or before it
    assert oracle.deskew(np.zeros((0, 3)), np.zeros(0), st)[1] == 0


def test_golden_frame_fixture_is_hermetic(oracle):
    """tests/golden/frame_small.npz: a stored 700-point sweep, its IMU states, and what deskew and scan
    preparation make of it (regression for the oracle; the GPU suite checks the device against it)."""
    g = np.load(os.path.join(GOLDEN, "frame_small.npz"))
    desk, moved = oracle.deskew(g["points"], g["point_time"], g["states"])
    assert moved == int(g["moved"]) and np.array_equal(desk, g["deskewed"])
    kp, kc, ki = oracle.preprocess(desk, float(g["voxel_size"]), int(g["knn"]))
    assert np.array_equal(ki, g["kept_index"]) and np.array_equal(kp, g["kept_points"])
    assert np.array_equal(kc, g["kept_covs"])
    npts, ncov, nidx = npo.preprocess(g["deskewed"], float(g["voxel_size"]), int(g["knn"]))
    assert np.array_equal(nidx, g["kept_index"].astype(np.int64))
    assert np.abs(ncov - g["kept_covs"].reshape(-1, 3, 3).transpose(0, 2, 1)).max() < 1e-10


def test_oracle_reproduces_the_degenerate_fixture(oracle):
    g = np.load(os.path.join(GOLDEN, "prep_degenerate.npz"))
    kp, kc, ki, bad = oracle.preprocess_ex(g["points"], float(g["voxel_size"]), int(g["knn"]))
    assert np.array_equal(ki, g["kept_index"]) and np.array_equal(kc, g["kept_covs"]) and bad == int(g["indefinite"]) > 0


def test_reference_hash_order_of_the_down_sampling_and_what_it_changes_downstream(oracle):
    """The reference emits the down-sampled scan in the iteration order of its std::unordered_map
    (src/CloudPreprocessor.cpp:94-99); oracle and HIP path emit ascending input index.  Voxel::addPoint is
    order-dependent (include/ESKF_LIO/LocalMap.hpp:79-87), so the map a real run builds differs.  This test states HOW
    MUCH on a 30-frame synthetic drive: the kept SET and every covariance are the same per frame, only the sequence
    differs; the two trajectories stay within the north-star tolerance of each other (measured 3e-5 m here, the
    number DESIGN.md quotes), with the same Gauss-Newton round counts."""
    from eskf_lio_amd import synth
    frames, n, cap = 30, 8_000, 20
    world = synth.make_lidar_scan(n, seed=0x46524D, extent=12.0)
    truth = [synth.se3_to_SE3([0.05 * f, 0.02 * f, 0.0, 0.0, 0.0, 0.004 * f]) for f in range(frames + 1)]

    def drive(order):
        rng = np.random.default_rng(12)
        omap = oracle.OracleMap(0.3, cap)
        pose, poses, kept = np.eye(4), [], []
        for f in range(frames + 1):
            Tinv = synth.invert_pose(truth[f])
            sweep = np.ascontiguousarray((world + rng.normal(scale=0.005, size=world.shape)) @ Tinv[:3, :3].T + Tinv[:3, 3])
            p, c, ix = oracle.preprocess_ordered(sweep, 0.3, 30, order)
            kept.append((p, c, ix))
            if f > 0:
                r = omap.align(p, c, pose, 30, 1e-6, 0.9999)
                pose = r.pose
                poses.append((pose.copy(), r.iterations))
            wp, wc = oracle.transform(p, c, pose)
            omap.insert(wp, wc)
        return poses, kept, len(omap)

    asc, kept_a, voxels_a = drive(oracle.ORDER_ASCENDING)
    ref, kept_r, voxels_r = drive(oracle.ORDER_REFERENCE_HASH)
    # frame 0 sees identical input both ways: same kept set, same covariances, another sequence
    (pa, ca, ia), (pr, cr, ir) = kept_a[0], kept_r[0]
    assert not np.array_equal(ia, ir) and np.array_equal(np.sort(ia), np.sort(ir))
    back = np.argsort(ir)
    assert np.array_equal(pa, pr[back]) and np.array_equal(ca, cr[back])
    assert np.array_equal(ia, np.sort(ia))                                       # ascending really is ascending
    p0, c0, i0 = oracle.preprocess(world, 0.3, 30)                               # the default entry point = ascending
    p1, c1, i1 = oracle.preprocess_ordered(world, 0.3, 30, oracle.ORDER_ASCENDING)
    assert np.array_equal(i0, i1) and np.array_equal(p0, p1) and np.array_equal(c0, c1)
    gap = max(float(np.linalg.norm(a[0][:3, 3] - b[0][:3, 3])) for a, b in zip(asc, ref))
    rot = max(pose_error(a[0], b[0])[1] for a, b in zip(asc, ref))
    print(f"\nreference hash order vs ascending over {frames} frames: trajectories differ by at most {gap:.2e} m / {rot:.2e} rad, "
          f"maps hold {voxels_a} vs {voxels_r} voxels")
    assert all(a[1] == b[1] for a, b in zip(asc, ref))                           # same round counts every frame
    assert 0.0 < gap < 1e-4 and rot < 1e-4                                       # a real effect, inside the tolerance
    assert abs(voxels_a - voxels_r) <= 0.002 * voxels_a
    for poses in (asc, ref):                                                     # both track the generating motion
        assert max(float(np.linalg.norm(p[0][:3, 3] - t[:3, 3])) for p, t in zip(poses, truth[1:])) < 5e-3
