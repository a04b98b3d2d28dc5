"""The pose prior (include/vgicp_hip_prior.h) without a device: the header and the exports, the host chart
(vgicp_pose_prior_chart, the kernels' own source) against tests/prior_reference.py's numpy restatement and against finite
differences, the iterated filter update of eskf_lio_amd/replay.py against the plain Kalman update on a linear model, and
the two native programs (the host plan with a prior set, the shim's new members)."""
import os
import re
import subprocess

import numpy as np
import pytest

import prior_reference as pr
import solver_reference as sr
from eskf_lio_amd import capi, replay
from test_evaluate_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACK = float(np.arccos(-0.9))                     # where so3_log hands over to so3_log_near_pi
# both sides of cosine = 0 (front / back half of the angle) and of cosine = -0.9
EDGE_THETAS = (0.5 * np.pi * (1 - 1e-12), 0.5 * np.pi * (1 + 1e-12), BACK * (1 - 1e-12), BACK * (1 + 1e-12))
THETAS = (0.0, 1e-9, 1e-6, 1e-3, 1.0, 3.1) + EDGE_THETAS
EPS = np.finfo(np.float64).eps
# What Log costs at most, in place of the 1 / sin(theta) of the tolerances below: so3_log divides by sin(theta) only while
# cosine > -0.9, where 1 / sin <= 1 / sqrt(1 - 0.81) = 2.294.  Beyond, so3_log_near_pi takes a_K = sqrt((M_KK - cos) /
# (1 - cos)) of the largest diagonal entry, a_K^2 >= 1/3 and 1 - cos >= 1.9: the quotient carries at most 2 eps / 1.9, the
# square root multiplies by 1 / (2 a_K) <= 0.87, and the two other entries divide a sum of two matrix entries by
# (1 - cos) a_K >= 1.097 — every factor below 2.294, and none grows towards pi.
LOG_COST_CAP = 1.0 / np.sqrt(1.0 - 0.81)


def log_cost(theta):
    s = np.sin(theta)
    return min(1.0 / s, LOG_COST_CAP) if s > 0.0 else LOG_COST_CAP


def random_pair(rng, theta):
    """(T0, T): a random prior pose and a pose whose rotation differs from it by exactly theta about a random axis."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    T0, T = np.eye(4), np.eye(4)
    T0[:3, :3] = pr.so3_exp(rng.uniform(-1.0, 1.0, size=3) * 2.0)
    T0[:3, 3] = rng.normal(size=3) * 3.0
    T[:3, :3] = T0[:3, :3] @ pr.so3_exp(theta * axis)
    T[:3, 3] = rng.normal(size=3) * 3.0
    return T0, T


def se3_exp(xi):
    """se3ToSE3 in closed form (R = Exp(omega), t = J_l(omega) v), the series of J_l below 1e-4 rad."""
    v, w = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    K = pr.hat(w)
    if th < 1e-4:
        J = np.eye(3) + 0.5 * K + K @ K / 6.0
    else:
        J = np.eye(3) + (1.0 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    T = np.eye(4)
    T[:3, :3] = pr.so3_exp(w)
    T[:3, 3] = J @ v
    return T


# ---- the header --------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_two_functions_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "vgicp_hip_prior.h")).read()
    assert '#include "vgicp_hip.h"' in text
    names = sorted(set(re.findall(r"^int\s+(vgicp_[a-z_0-9]+)\s*\(", text, flags=re.M)))
    assert names == sorted(capi.PRIOR_EXPORTS) == ["vgicp_pose_prior_chart", "vgicp_set_pose_prior"]
    assert re.search(r"int vgicp_set_pose_prior\(vgicp_ctx\* ctx, const double prior_pose\[16\], const double information\[36\]\);", text)
    assert re.search(r"int vgicp_pose_prior_chart\(const double prior_pose\[16\], const double pose\[16\], double d\[6\], "
                     r"double G\[36\]\);", text)
    # every vgicp_ name followed by "(" in the header is one of the two or an entry point of another header (prose)
    assert set(names) <= set(declared("vgicp_hip_prior.h"))
    lib = capi.load_library()
    # the library of this header, beside the module (whose own exports stay the pinned lists): exactly the two
    assert os.path.dirname(capi.side_lib_path("prior")) == os.path.dirname(capi.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("prior")], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert exported == set(names)
    for name in names:
        assert hasattr(lib, name), name
    assert "libvgicp_hip_prior.so" in text
    # the main header's list stays pinned at 47, the ABI version at 6
    main = declared("vgicp_hip.h")
    assert len(main) == 47 and sorted(capi.EXPORTS) == main and not set(main) & set(names)
    assert lib.vgicp_abi_version() == 6
    # what the header must say: the chart, the scope, what the log keeps
    for phrase in ("Log(R0^T R)", "G^T L G", "DATA sums", "no fused upload", "hypotheses_per_launch = 1",
                   "vgicp_create_multi", "positive semi-definite", "1e-12", "1e-9"):
        assert phrase in text, phrase


def test_calls_without_a_context_or_a_pose():
    lib = capi.load_library()
    eye, info = capi.pose_to_abi(np.eye(4)), np.eye(6).reshape(36)
    assert lib.vgicp_set_pose_prior(None, capi._dp(eye), capi._dp(info)) == capi.ERR_BAD_ARGUMENT
    d, G = np.zeros(6), np.zeros(36)
    assert lib.vgicp_pose_prior_chart(None, capi._dp(eye), capi._dp(d), capi._dp(G)) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_pose_prior_chart(capi._dp(eye), None, capi._dp(d), capi._dp(G)) == capi.ERR_BAD_ARGUMENT
    bad = eye.copy()
    bad[12] = np.nan
    assert lib.vgicp_pose_prior_chart(capi._dp(eye), capi._dp(bad), capi._dp(d), capi._dp(G)) == capi.ERR_BAD_ARGUMENT
    # either output may be NULL
    assert lib.vgicp_pose_prior_chart(capi._dp(eye), capi._dp(eye), None, capi._dp(G)) == capi.OK
    assert lib.vgicp_pose_prior_chart(capi._dp(eye), capi._dp(eye), capi._dp(d), None) == capi.OK
    assert np.array_equal(G.reshape(6, 6), np.eye(6)) and not d.any()


def test_a_context_of_another_build_is_refused_untouched():
    """vgicp_set_pose_prior writes fields of the module's context from a library of its own: the first eight bytes of a
    context are the creating module's layout stamp, and anything else there (here: a block that no module created) is
    refused before a byte of it is read or written, for a set and for a clear, with the text at vgicp_last_error(NULL)."""
    import ctypes as C
    lib = capi.load_library()
    eye, info = capi.pose_to_abi(np.eye(4)), np.eye(6).reshape(36)
    for first in (0, 0x7667637000000000, 0x7667637000000000 | 8):
        block = (C.c_uint64 * 8)(first, *([0xA5A5A5A5A5A5A5A5] * 7))
        before = bytes(block)
        assert lib.vgicp_set_pose_prior(C.addressof(block), capi._dp(eye), capi._dp(info)) == capi.ERR_BAD_ARGUMENT
        assert b"not from one build" in lib.vgicp_last_error(None)
        assert lib.vgicp_set_pose_prior(C.addressof(block), None, None) == capi.ERR_BAD_ARGUMENT
        assert bytes(block) == before


# ---- the chart ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", THETAS)
def test_chart_equals_the_numpy_restatement(theta):
    """d and G of vgicp_pose_prior_chart against prior_reference.chart (the header's equations in numpy, its own Log).
    Both are a few dozen fp64 operations on entries of size S = 1 + |t| + theta; Log divides by sin(theta), which costs
    1 / sin(3.1) = 24 at the largest angle: 64 eps x 24 x S covers it (observed: 9e-16 at 3.1, 1e-16 elsewhere)."""
    rng = np.random.default_rng(int(theta * 1000) + 7)
    worst = 0.0
    for _ in range(50):
        T0, T = random_pair(rng, theta)
        d, G = capi.pose_prior_chart(T0, T)
        d_ref, G_ref = pr.chart(T0, T)
        S = 1.0 + np.linalg.norm(T[:3, 3]) + theta
        tol = 64 * EPS * 24 * S
        worst = max(worst, np.abs(d - d_ref).max(), np.abs(G - G_ref).max())
        assert np.abs(d - d_ref).max() <= tol and np.abs(G - G_ref).max() <= tol
        assert abs(np.linalg.norm(d[3:]) - theta) <= tol
        assert np.array_equal(G[:3, :3], np.eye(3)) and not G[3:, :3].any()
        # Jr^-1(phi) phi = phi: the lower right block is Jr^-1 R^T
        Jr_inv = G[3:, 3:] @ T[:3, :3]
        assert np.abs(Jr_inv @ d[3:] - d[3:]).max() <= tol
    print(f"theta {theta}: worst difference {worst:.3e}")


@pytest.mark.parametrize("theta", THETAS)
def test_jacobian_equals_the_central_difference(theta):
    """G against (d(se3ToSE3(+h e_k) T) - d(se3ToSE3(-h e_k) T)) / 2h, all in numpy.  Step and tolerance from the
    difference's own error: truncation h^2 / 6 x |third derivative| and rounding eps x |d| / h.  d's entries and its
    derivatives in xi are of size S = 1 + |t| + theta (t' = Exp(omega) t + J v; Log and Jr^-1 are smooth up to 2 pi), so
    with h = 1e-5 the two parts are 1.7e-11 S and 2.2e-11 S; the bound is (2 h^2 + 4 eps / h) S = 2.9e-10 S, a factor of
    a few above their sum."""
    h = 1e-5
    rng = np.random.default_rng(int(theta * 1000) + 11)
    worst = 0.0
    for _ in range(20):
        T0, T = random_pair(rng, theta)
        _, G = capi.pose_prior_chart(T0, T)
        S = 1.0 + np.linalg.norm(T[:3, 3]) + theta
        tol = (2 * h * h + 4 * EPS / h) * S
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            plus, _ = pr.chart(T0, se3_exp(e) @ T)
            minus, _ = pr.chart(T0, se3_exp(-e) @ T)
            column = (plus - minus) / (2 * h)
            worst = max(worst, np.abs(column - G[:, k]).max() / S)
            assert np.abs(column - G[:, k]).max() <= tol, (theta, k)
    print(f"theta {theta}: worst |FD - G| / S {worst:.3e}")


@pytest.mark.skipif(sr.unavailable_reason() is not None, reason=str(sr.unavailable_reason()))
@pytest.mark.parametrize("theta", EDGE_THETAS + (3.1, np.pi - 1e-8))
def test_chart_at_the_branch_edges_equals_extended_precision(theta):
    """d and G at the angles where so3_log changes its formula, and 1e-8 below pi, against tests/solver_reference.py: Log
    of the very fp64 matrices the library receives and Jr^-1 in extended precision (prior_reference's c(theta) cannot
    serve next to pi: its closed form has the pole the header's second form avoids).  The tolerance formula of
    test_chart_equals_the_numpy_restatement, 64 eps x (cost of Log) x S, the cost 1 / sin(theta) capped by what the
    near-pi branch costs itself (LOG_COST_CAP above, with its derivation): at pi - 1e-8 that is 2.3 in place of 1e8.
    The angle and the axis come back as they went in (observed: 0.014 of the tolerance at worst, at pi / 2)."""
    rng = np.random.default_rng(int(theta * 1000) + 13)
    worst = 0.0
    for _ in range(50):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        T0, T = random_pair(rng, 0.0)
        unit = axis.astype(sr.LD)
        unit /= np.sqrt(unit @ unit)
        T[:3, :3] = np.asarray(T0[:3, :3].astype(sr.LD) @ sr.so3_exp(theta, unit), dtype=np.float64)
        d, G = capi.pose_prior_chart(T0, T)
        d_ref, G_ref = sr.chart(T0, T)
        tol = 64 * EPS * log_cost(theta) * (1.0 + np.linalg.norm(T[:3, 3]) + theta)
        diff = max(float(np.abs(d - d_ref).max()), float(np.abs(G - G_ref).max()))
        worst = max(worst, diff / tol)
        assert diff <= tol, (theta, diff, tol)
        assert abs(np.linalg.norm(d[3:]) - theta) <= tol and np.abs(d[3:] - theta * axis).max() <= tol
        Jr_inv = G[3:, 3:] @ T[:3, :3]
        assert np.abs(Jr_inv @ d[3:] - d[3:]).max() <= tol
    print(f"theta {theta}: worst difference / tolerance {worst:.3e}")


@pytest.mark.skipif(sr.unavailable_reason() is not None, reason=str(sr.unavailable_reason()))
@pytest.mark.parametrize("K", (0, 1, 2))
def test_chart_at_exactly_pi(K):
    """R0^T R = diag(1, -1, -1) and its two permutations, exactly: R0 a signed permutation matrix, so the product is
    exact too.  The sine is zero and either sign of phi is the Log: Exp(phi) is compared with R0^T R, |phi| with pi, and G
    with the extended-precision chart of the sign that came back.  Tolerance as above (cost LOG_COST_CAP); Exp(phi) is
    off the matrix by pi - fl(pi) = 1.2e-16 on top of its own rounding."""
    half_turn = -np.ones(3)
    half_turn[K] = 1.0
    for R0 in (np.eye(3), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
               np.array([[0.0, 0.0, 1.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]])):
        assert np.linalg.det(R0) == 1.0
        T0, T = np.eye(4), np.eye(4)
        T0[:3, :3], T[:3, :3] = R0, R0 @ np.diag(half_turn)
        T0[:3, 3], T[:3, 3] = [0.5, -1.0, 2.0], [1.5, 0.25, -3.0]
        assert np.array_equal(T0[:3, :3].T @ T[:3, :3], np.diag(half_turn))
        d, G = capi.pose_prior_chart(T0, T)
        phi = d[3:]
        tol = 64 * EPS * LOG_COST_CAP * (1.0 + np.linalg.norm(T[:3, 3]) + np.pi)
        assert np.array_equal(d[:3], T[:3, 3] - T0[:3, 3])
        assert abs(abs(phi[K]) - np.pi) <= tol and np.abs(np.delete(phi, K)).max() <= tol, phi
        angle = np.sqrt(phi.astype(sr.LD) @ phi.astype(sr.LD))
        back = sr.so3_exp(angle, phi.astype(sr.LD) / angle)
        assert np.abs(np.asarray(back, dtype=np.float64) - np.diag(half_turn)).max() <= tol
        exact = np.zeros(3, dtype=sr.LD)
        exact[K] = np.sign(phi[K]) * sr.PI                       # the Log of that sign, to extended precision
        d_ref, G_ref = sr.chart(T0, T, exact)
        assert float(np.abs(d - d_ref).max()) <= tol and float(np.abs(G - G_ref).max()) <= tol
        assert np.array_equal(G[:3, :3], np.eye(3)) and not G[3:, :3].any()


def test_series_switch_over_is_the_exponentials():
    """c(theta) takes its series up to theta^2 = 0.25, where se3_exp_device leaves its own; the two forms meet there."""
    math_h = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "vgicp_math.h")).read()
    kernels = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "vgicp_kernels.hip")).read()
    assert re.search(r"constexpr double kJrSeriesMax2 = 0\.25;", math_h) and "if (n2 > kJrSeriesMax2)" in math_h
    body = kernels[kernels.index("void se3_exp_device("):]
    assert re.search(r"if \(n2 > 0\.25\) \{", body[:600])
    assert pr.SERIES_MAX2 == 0.25 and abs(pr.C_SERIES[0] - 1.0 / 12.0) < 1e-18
    th = 0.5
    closed = 1.0 / th ** 2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    assert abs(pr.c_theta(th) - closed) <= 64 * EPS          # the closed form cancels 4 - 3.92 there: ~50 eps
    assert pr.c_theta(0.0) == 1.0 / 12.0
    # the library on both sides of the switch-over, against the numpy chart (which switches at the same place)
    rng = np.random.default_rng(5)
    for theta in (0.5 * (1 - 1e-12), 0.5 * (1 + 1e-12)):
        T0, T = random_pair(rng, theta)
        _, G = capi.pose_prior_chart(T0, T)
        _, G_ref = pr.chart(T0, T)
        assert np.abs(G - G_ref).max() <= 256 * EPS * (1.0 + np.linalg.norm(T[:3, 3]))


# ---- the replay's iterated update --------------------------------------------------------------------------------------
def test_iterated_update_is_the_kalman_update_on_a_linear_model():
    """ErrorStateKF.update with kalman_filter.update.iterated against the plain Kalman update with V = A_c^-1, the align
    stubbed by an exactly linear model: data information A_c and data optimum z_obs in the filter's chart, so the MAP
    residual is z* = (L + A_c)^-1 A_c z_obs and the posterior information A_c + L.  dx and P+ to 1e-10 relative."""
    rng = np.random.default_rng(9)
    B = rng.normal(size=(6, 6))
    A_c = 2.0e3 * (B @ B.T + 6.0 * np.eye(6))
    z_obs = np.array([0.03, -0.02, 0.01, 0.004, -0.006, 0.005])
    seen = {}

    def stub(points, covs, guess, information):
        z = np.linalg.solve(information + A_c, A_c @ z_obs)
        T = np.eye(4)
        T[:3, 3] = guess[:3, 3] + z[:3]
        T[:3, :3] = guess[:3, :3] @ pr.so3_exp(z[3:])
        seen["information"] = information.copy()
        return T, A_c + information

    config = dict(replay.DEFAULT_CONFIG, kalman_filter=dict(replay.DEFAULT_CONFIG["kalman_filter"], iterated=True))
    assert "iterated" not in replay.DEFAULT_CONFIG["kalman_filter"]          # default off
    with pytest.raises(ValueError):
        replay.ErrorStateKF(config, align=None)                             # the iterated update needs the prior align
    kf = replay.ErrorStateKF(config, align=None, align_with_prior=stub)
    kf.initialize(0.0)
    for k in range(1, 41):                                                  # 0.1 s of prediction so that P is full
        kf.process(replay.ImuMeasurement(k / 400.0, 0.05 * rng.normal(size=3),
                                         np.array([0.0, 0.0, -9.805]) + 0.1 * rng.normal(size=3)))
    prior = kf.getStates()[-1].copy()
    lidar = replay.LidarMeasurement(np.zeros((1, 3)), np.array([0.1]))
    lidar.covariances = np.zeros((1, 9))
    lidar.endTime = 0.1
    kf.update(lidar)
    err, P_plus = kf.last_correction
    H, P = kf.H_, prior.P
    S = H @ P @ H.T
    assert np.allclose(seen["information"], np.linalg.inv(S), rtol=1e-9, atol=0)
    K = P @ H.T @ np.linalg.inv(S + np.linalg.inv(A_c))
    err_ref, P_ref = K @ z_obs, (np.eye(18) - K @ H) @ P
    d_err = np.abs(err - err_ref).max() / np.abs(err_ref).max()
    d_P = np.abs(P_plus - P_ref).max() / np.abs(P_ref).max()
    print(f"dx {d_err:.3e}, P+ {d_P:.3e} relative")
    assert d_err <= 1e-10 and d_P <= 1e-10
    # and the plain update is untouched by the new key being absent or false
    plain = replay.ErrorStateKF(dict(replay.DEFAULT_CONFIG, kalman_filter=dict(replay.DEFAULT_CONFIG["kalman_filter"],
                                                                                   iterated=False)), align=lambda p, c, g: g)
    assert not plain.iterated_
    src = open(os.path.join(ROOT, "tools", "replay.py")).read()
    assert "--prior-update" in src


# ---- the native programs -----------------------------------------------------------------------------------------------
def test_align_plan_with_a_prior_is_the_robust_rounds_plan(tmp_path):
    """tests/native/align_plan_prior.cpp: over the facts tests/native/align_plan_robust.cpp enumerates, the plan with
    prior = true (and with prior and robust) is the plan with robust = true: same path, width and cool-down."""
    exe = tmp_path / "align_plan_prior"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "align_plan_prior.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 84_934_656, run.stdout
    counts = dict(zip(words[3::2], map(int, words[4::2])))
    assert counts["fused"] == 0 and counts["teams"] == 0
    assert counts["persistent"] > 0 and counts["loop"] > 0 and counts["group-loop"] > 0


def test_shim_members_compile_against_the_stubs(tmp_path):
    """tests/native/shim_prior.cpp: ICP::setPrior / clearPrior / alignWithPrior / posteriorInformation with the issue's
    signatures against the stand-in types, align's own signature unchanged, and the bookkeeping that needs no device."""
    exe = tmp_path / "shim_prior"
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "tests", "compile_native", "stubs"), "-I" + os.path.join(ROOT, "include"),
                          "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_prior.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout[-1000:] + run.stderr[-500:]
