"""The per-point report (include/vgicp_hip_points.h) without a device: the header against the Python mirror, the two
libraries' exports, the host plan (refusal order, ranks, sort keys), the shim's scale from a quantile, the replay flag,
and the preconditions of tests/test_points.py, checked on the reference alone."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import points_reference as pr
import robust_reference as rr
from eskf_lio_amd import capi
from test_evaluate_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY_FIELDS = ("points", "matched", "counted", "negative", "not_finite", "quantile")
STATS_FIELDS = ("launches", "reserved", "seconds", "device_seconds")


# ---- header and libraries ---------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_its_library_exports_it():
    lib = capi.load_library()
    assert declared("vgicp_hip_points.h") == sorted(capi.POINTS_EXPORTS) == ["vgicp_points_resident"]
    text = open(os.path.join(ROOT, "include", "vgicp_hip_points.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_points.so" in text

    def define(name):
        m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, text)
        assert m, name
        return int(m.group(1))

    assert define("VGICP_POINT_QUANTILES_MAX") == capi.POINT_QUANTILES_MAX == 16
    assert (define("VGICP_POINT_MATCHED"), define("VGICP_POINT_NEGATIVE"), define("VGICP_POINT_NOT_FINITE")) == \
        (capi.POINT_MATCHED, capi.POINT_NEGATIVE, capi.POINT_NOT_FINITE) == (1, 2, 4)
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("points")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.POINTS_EXPORTS)
    assert hasattr(lib, "vgicp_points_resident")
    # the UNITS paragraph of the robust header points here
    robust = open(os.path.join(ROOT, "include", "vgicp_hip_robust.h")).read()
    assert "vgicp_hip_points.h" in robust and "vgicp_points_resident" in robust


def test_module_still_exports_exactly_the_four_pinned_lists():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    pinned = set(capi.EXPORTS) | set(capi.MAP_POINTS_EXPORTS) | set(capi.BATCH_EXPORTS) | set(capi.EVALUATE_EXPORTS)
    assert len(pinned) == 47 + 2 + 2 + 1 and exported == pinned
    assert not set(capi.POINTS_EXPORTS) & pinned and len(capi.EXPORTS) == 47
    assert lib.vgicp_abi_version() == 6


def test_layouts_match_the_header(tmp_path):
    assert C.sizeof(capi.PointSummary) == 168 and C.sizeof(capi.PointStats) == 24
    assert [f for f, _ in capi.PointSummary._fields_] == list(SUMMARY_FIELDS)
    assert [f for f, _ in capi.PointStats._fields_] == list(STATS_FIELDS)
    assert [getattr(capi.PointSummary, f).offset for f in SUMMARY_FIELDS] == [0, 8, 16, 24, 32, 40]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_points.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vgicp_point_summary));\n' +
                   "".join(f'  printf(" %zu", offsetof(vgicp_point_summary, {f}));\n' for f in SUMMARY_FIELDS) +
                   '  printf(" %zu", sizeof(vgicp_point_stats));\n' +
                   "".join(f'  printf(" %zu", offsetof(vgicp_point_stats, {f}));\n' for f in STATS_FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == ([168] + [getattr(capi.PointSummary, f).offset for f in SUMMARY_FIELDS] +
                   [24] + [getattr(capi.PointStats, f).offset for f in STATS_FIELDS])


def test_entry_point_refuses_a_null_context_and_a_foreign_one_and_writes_nothing():
    lib = capi.load_library()
    pose = (C.c_double * 16)(*np.eye(4).reshape(16))
    summary = capi.PointSummary()
    C.memset(C.byref(summary), 0xA5, C.sizeof(summary))
    before = bytes(summary)
    assert lib.vgicp_points_resident(None, pose, 0, None, None, None, None, 0, None, C.byref(summary), None) == \
        capi.ERR_BAD_ARGUMENT
    # a block that no build of the module stamped: refused by the handshake, which reads its first word only
    foreign = C.create_string_buffer(4096)
    assert lib.vgicp_points_resident(C.cast(foreign, C.c_void_p), pose, 0, None, None, None, None, 0, None,
                                     C.byref(summary), None) == capi.ERR_BAD_ARGUMENT
    assert "not from one build" in lib.vgicp_last_error(None).decode()
    assert bytes(summary) == before and foreign.raw == bytes(4096)


# ---- the host plan ----------------------------------------------------------------------------------------------------
RANK_M = (0, 1, 2, 255, 256, 257, 5856, 2 ** 31 - 1)
RANK_Q = (0.0, 1e-12, 0.25, 0.5, 0.9, 0.99, 1.0 - 2.0 ** -53, 1.0)


def test_points_plan(tmp_path):
    """tests/native/points_plan.cpp: the refusal order over every combination of the facts against the header's list; the
    rank of every (m, q) below against the formula in Python integers and math.ceil (m = 0 has no rank: 0 by
    convention, the caller reports NaN); the sort key's order."""
    exe = tmp_path / "points_plan"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "points_plan.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    lines = run.stdout.splitlines()
    assert lines[0] == "plan ok %d" % (4096 * 4 * 5) and lines[-1] == "keys ok"
    ranks = {(int(m), int(j)): int(r) for _, m, j, r in (line.split() for line in lines if line.startswith("rank "))}
    assert len(ranks) == len(RANK_M) * len(RANK_Q)
    for m in RANK_M:
        for j, q in enumerate(RANK_Q):
            want = min(max(math.ceil(q * m), 1), m) - 1 if m else 0
            assert ranks[(m, j)] == want == (pr.quantile_rank(q, m) if m else 0), (m, q, ranks[(m, j)], want)
    # what the formula means at its ends: the smallest value for q = 0, the largest for q = 1 and just below
    assert ranks[(5856, 0)] == 0 and ranks[(5856, 7)] == 5855 and ranks[(5856, 6)] == 5855 and ranks[(5856, 3)] == 2927
    assert ranks[(2 ** 31 - 1, 7)] == 2 ** 31 - 2 and ranks[(1, 3)] == 0


def test_shim_scale_from_quantile(tmp_path):
    """tests/native/shim_points.cpp against the stand-in types: robustScaleFromQuantile's values and refusals."""
    exe = tmp_path / "shim_points"
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
           "-I" + os.path.join(ROOT, "tests", "compile_native", "stubs"), "-I" + os.path.join(ROOT, "include"),
           "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_points.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout[-1000:] + run.stderr[-500:]


def test_replay_passes_the_quantile_through():
    """tools/replay.py's --robust-scale-quantile ends up as registration.robust_scale_quantile; off by default."""
    src = open(os.path.join(ROOT, "tools", "replay.py")).read()
    assert "--robust-scale-quantile" in src and '"robust_scale_quantile", args.robust_scale_quantile' in src
    from eskf_lio_amd import replay
    assert "robust_scale_quantile" not in replay.DEFAULT_CONFIG["registration"]
    assert replay.robust_scale_from_quantile(0.0625) == 0.25
    assert replay.robust_scale_from_quantile(float("nan")) is None
    assert replay.robust_scale_from_quantile(0.0) == 1e-6 and replay.robust_scale_from_quantile(1e12) == (2 ** 31 - 1) / 1e6


# ---- preconditions of tests/test_points.py, on the reference alone ------------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle):
    vmap, pts, covs, T_true, guess = rr.make_scene()
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    return om, pts, covs, T_true, guess


def test_preconditions_of_the_gpu_tests(scene, oracle):
    """No rank and no gate decision of tests/test_points.py can hang on a rounding: neighbouring sorted d^2 are at least
    1e-7 apart (relative) and every gate is more than 1e-9 from the nearest d^2, both beyond the device's per-term bound
    of 72 kappa^2 u ~ 8e-11."""
    om, pts, covs, T_true, guess = scene
    at_true, at_guess = (pr.reference_at(oracle, om, pts, covs, pose) for pose in (T_true, guess))
    assert at_true.n == 6000 and len(at_true.index) == 5856 and len(at_guess.index) == 5905
    bound = pr.COST_C * 100.0001 ** 2 * pr.U
    assert 7.9e-11 < bound < 8.1e-11
    for name, ref in (("T_true", at_true), ("guess", at_guess)):
        assert not (ref.raw < 0.0).any() and np.isfinite(ref.raw).all() and ref.kappa <= 100.0001
        assert (ref.raw > 0.0).all() and np.isfinite(ref.sq).all()
        gap = pr.smallest_relative_gap(ref.ranked)
        margins = [pr.gate_margin(ref.raw, g) for g in pr.GATES]
        print(f"{name}: smallest relative gap {gap:.3e}, gate margins {['%.3e' % v for v in margins]}, kappa {ref.kappa!r}")
        assert gap >= 1e-7 > bound and min(margins) > 1e-9 > bound
    assert "%.1e" % pr.smallest_relative_gap(at_true.ranked) == "1.7e-07"
    assert "%.1e" % pr.smallest_relative_gap(at_guess.ranked) == "2.1e-07"
    assert "%.1e" % pr.gate_margin(at_guess.raw, 0.01) == "3.4e-05"


def test_reference_scale_from_a_quantile_meets_the_robust_criterion(scene, oracle):
    """Huber with c = sqrt(a quantile of d^2 at the guess) on the reference IRLS.  The 0.9 quantile (0.066, c = 0.257)
    does NOT halve the plain align's translation error on this scene (10.8 mm against 16.1 mm: a tenth of the points keep
    a reduced weight only, and a fifth are displaced); the median (0.0079, c = 0.089) does (5.1 mm), so the median is
    what tests/test_points.py puts through the shim."""
    om, pts, covs, T_true, guess = scene
    ranked = pr.reference_at(oracle, om, pts, covs, guess).ranked
    plain = rr.translation_error(rr.irls_align(oracle, om, pts, covs, guess).pose, T_true)
    errors = {}
    for q in (0.9, 0.5):
        c = round(math.sqrt(pr.order_statistics(ranked, [q])[0]) * 1e6) / 1e6
        got = rr.irls_align(oracle, om, pts, covs, guess, rr.HUBER, c, 0.0)
        errors[q] = rr.translation_error(got.pose, T_true)
        print(f"quantile {q}: c {c}, rounds {got.iterations}, error {1e3 * errors[q]:.3f} mm against {1e3 * plain:.3f} mm")
        assert got.converged
    assert "%.3f" % math.sqrt(pr.order_statistics(ranked, [0.9])[0]) == "0.257"
    assert errors[0.9] > 0.5 * plain and errors[0.5] <= 0.5 * plain
