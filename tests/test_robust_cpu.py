"""Robust rounds (include/vgicp_hip_robust.h) without a device: the header against the Python mirror, the pinned export
lists, the host plan with the mode on, the shim's settings, and the reference IRLS that tests/test_robust.py holds the
GPU against."""
import os
import re
import subprocess

import numpy as np
import pytest

import robust_reference as rr
from eskf_lio_amd import capi
from test_evaluate_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_python_mirror_and_declares_no_function():
    text = open(os.path.join(ROOT, "include", "vgicp_hip_robust.h")).read()
    assert '#include "vgicp_hip.h"' in text

    def define(name):
        m = re.search(r"#define\s+%s\s+(-?\d+)\b" % name, text)
        assert m, name
        return int(m.group(1))

    assert (define("VGICP_OPTION_ROBUST_KERNEL"), define("VGICP_OPTION_ROBUST_SCALE_MICRO"),
            define("VGICP_OPTION_GATE_MICRO")) == (capi.OPTION_ROBUST_KERNEL, capi.OPTION_ROBUST_SCALE_MICRO,
                                                   capi.OPTION_GATE_MICRO) == (5, 6, 7)
    assert (define("VGICP_ROBUST_NONE"), define("VGICP_ROBUST_HUBER"), define("VGICP_ROBUST_CAUCHY")) == \
        (capi.ROBUST_NONE, capi.ROBUST_HUBER, capi.ROBUST_CAUCHY) == (0, 1, 2)
    # the numbers are free in the main header and in the other extension
    main = open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()
    taken = {int(v) for v in re.findall(r"#define\s+VGICP_OPTION_[A-Z_]+\s+(\d+)", main)}
    points = open(os.path.join(ROOT, "include", "vgicp_hip_map_points.h")).read()
    taken |= {int(v) for v in re.findall(r"#define\s+VGICP_OPTION_[A-Z_]+\s+(\d+)", points)}
    assert taken == {1, 2, 3, 4}
    assert declared("vgicp_hip_robust.h") == [] == sorted(capi.ROBUST_EXPORTS)
    # what the header must say: the units, where to look d^2 up, and the limits
    for phrase in ("REGULARISED", "vgicp_evaluate_resident", "UNWEIGHTED", "single-device", "vgicp_create_multi",
                   "hypotheses_per_launch = 1", "no fused upload"):
        assert phrase in text, phrase


def test_library_still_exports_exactly_the_four_pinned_lists():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    pinned = set(capi.EXPORTS) | set(capi.MAP_POINTS_EXPORTS) | set(capi.BATCH_EXPORTS) | set(capi.EVALUATE_EXPORTS)
    assert len(pinned) == 47 + 2 + 2 + 1 and exported == pinned
    assert lib.vgicp_abi_version() == 6


def test_options_are_refused_without_a_context():
    lib = capi.load_library()
    for option in (capi.OPTION_ROBUST_KERNEL, capi.OPTION_ROBUST_SCALE_MICRO, capi.OPTION_GATE_MICRO):
        assert lib.vgicp_set_option(None, option, 1) == capi.ERR_BAD_ARGUMENT


def test_align_plan_with_the_robust_round_on(tmp_path):
    """tests/native/align_plan_robust.cpp: over the facts tests/native/align_plan.cpp enumerates, with robust = true, no
    plan is Fused or Teams, width is 1, and every other field is the plain plan of the same facts with no_fused set and
    the batch taken as singles."""
    exe = tmp_path / "align_plan_robust"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "align_plan_robust.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 84_934_656, run.stdout
    counts = dict(zip(words[3::2], map(int, words[4::2])))
    assert counts["fused"] == 0 and counts["teams"] == 0
    assert counts["persistent"] > 0 and counts["loop"] > 0 and counts["group-loop"] > 0
    assert sum(counts.values()) == 84_934_656


@pytest.mark.parametrize("keys", [False, True], ids=["keys-absent", "keys-present"])
def test_shim_settings_compile_and_refuse_bad_values(tmp_path, keys):
    """tests/native/shim_robust.cpp against the stand-in types: the YAML constructor with the optional keys absent (the
    reference's file: the plain round) and present, setRobust's rounding to millionths, and its refusal of a bad kind,
    scale or gate, which changes nothing."""
    exe = tmp_path / "shim_robust"
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    if keys:
        cmd += ["-DKEYS_PRESENT", "-I" + os.path.join(ROOT, "tests", "native", "yaml_with_keys")]
    cmd += ["-I" + os.path.join(ROOT, "tests", "compile_native", "stubs"), "-I" + os.path.join(ROOT, "include"),
            "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_robust.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout[-1000:] + run.stderr[-500:]


def test_replay_passes_the_settings_through():
    """tools/replay.py's --robust-kernel / --robust-scale / --gate end up as registration.* keys; off by default."""
    src = open(os.path.join(ROOT, "tools", "replay.py")).read()
    for flag in ("--robust-kernel", "--robust-scale", "--gate"):
        assert flag in src
    from eskf_lio_amd import replay
    assert not {"robust_kernel", "robust_scale", "gate"} & set(replay.DEFAULT_CONFIG["registration"])


# ---- the reference IRLS ------------------------------------------------------------------------------------------------
# the issue's table: mode -> (rounds, translation error in mm to 3 significant figures, counts of round 0 and of the last
# round, correspondences before the gate in round 0 and in the last round)
TABLE = {
    "cauchy": (9, 3.59, 5905, 5867, 5905, 5867),
    "huber": (10, 4.94, 5905, 5871, 5905, 5871),
    "gate": (5, 1.07, 5002, 5127, 5905, 5859),
    "cauchy+gate": (11, 1.10, 5272, 5236, 5905, 5859),
}


@pytest.fixture(scope="module")
def scene(oracle):
    vmap, pts, covs, T_true, guess = rr.make_scene()
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    return om, pts, covs, T_true, guess


def test_reference_without_kernel_and_gate_is_the_oracles_align(scene, oracle):
    om, pts, covs, T_true, guess = scene
    ref = om.align(pts, covs, guess, rr.MAX_IT, rr.TSQ, rr.COS)
    got = rr.irls_align(oracle, om, pts, covs, guess)
    assert got.iterations == ref.iterations == 3 and got.converged and ref.converged
    assert np.array_equal(got.corr_count, ref.corr_count) and list(ref.corr_count[[0, -1]]) == [5905, 5907]
    assert np.abs(got.pose - ref.pose).max() <= 1e-15
    for it in range(3):
        assert np.array_equal(got.normal_eq[it], rr.packed(ref.JTJ[it], ref.JTr[it]))
    assert "%.2f" % (1e3 * rr.translation_error(ref.pose, T_true)) == "16.10"


@pytest.mark.parametrize("mode", list(TABLE))
def test_reference_reproduces_the_table(scene, oracle, mode):
    om, pts, covs, T_true, guess = scene
    kernel, c, gate = rr.MODES[mode]
    rounds, err_mm, first, last, matched_first, matched_last = TABLE[mode]
    got = rr.irls_align(oracle, om, pts, covs, guess, kernel, c, gate)
    err = 1e3 * rr.translation_error(got.pose, T_true)
    print(f"{mode}: rounds {got.iterations}, error {err:.4f} mm, counts {got.corr_count}, matched {got.matched}")
    assert got.converged and got.iterations == rounds
    assert float("%.3g" % err) == err_mm
    assert (int(got.corr_count[0]), int(got.corr_count[-1])) == (first, last)
    assert (int(got.matched[0]), int(got.matched[-1])) == (matched_first, matched_last)
    assert err <= 0.31 * 16.10          # what the mode is for: the plain align's error, more than halved


def test_weights_follow_the_header():
    d2 = np.array([-1e-18, 0.0, 0.0064, 0.0064000001, 0.04, 0.09, np.nan])
    w, clamped = rr.weights(d2, rr.HUBER, 0.08, 0.0)
    assert clamped[0] == 0.0 and list(w[:3]) == [1.0, 1.0, 1.0] and w[3] < 1.0
    assert abs(w[4] - 0.08 / 0.2) < 1e-16 and abs(w[5] - 0.08 / 0.3) < 1e-16
    w, _ = rr.weights(d2, rr.CAUCHY, 0.15, 0.06)
    assert w[0] == 1.0 and abs(w[4] - 1.0 / (1.0 + 0.04 / 0.0225)) < 1e-16
    assert w[5] == 0.0 and w[6] == 0.0                      # beyond the gate; a NaN residual is rejected
    w, _ = rr.weights(d2, rr.HUBER, 2147.483647, 0.0)       # the neutral mode
    assert list(w[:6]) == [1.0] * 6
