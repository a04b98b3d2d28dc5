"""Submap as scan (include/vgicp_hip_map_submap.h) without a device: the header against the Python mirror, the libraries'
exports, the struct layouts, the host plan (plan_submap's refusals in their order), the shim's new methods, the numpy
restatement of the rule on hand-worked cases, and the end-to-end recipe on the oracle alone: the basin condition that
tests/test_map_submap.py asks of the device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import map_submap_reference as ms
from eskf_lio_amd import capi, synth
from test_evaluate_cpu import declared
from test_map_gated_cpu import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS_FIELDS = ("center", "radius", "frame", "min_count", "level", "reserved")
STATS_FIELDS = ("voxels", "points", "too_far", "too_few", "launches", "reserved", "seconds", "device_seconds")


# ---- header and libraries ---------------------------------------------------------------------------------------------
def test_header_declares_the_two_functions_and_the_library_exports_them():
    lib = capi.load_library()
    assert declared("vgicp_hip_map_submap.h") == sorted(capi.MAP_SUBMAP_EXPORTS) == ["vgicp_scan_from_map", "vgicp_scan_from_map_keys"]
    assert capi.SIDE_EXPORTS["map_submap"] is capi.MAP_SUBMAP_EXPORTS
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_submap.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_map_submap.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("map_submap")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.MAP_SUBMAP_EXPORTS)
    assert all(hasattr(lib, name) for name in capi.MAP_SUBMAP_EXPORTS)
    assert re.findall(r"^ \*\s+(\d+)\. ", text, flags=re.M) == [str(k) for k in range(1, 12)]          # the eleven refusals
    makefile = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "Makefile")).read()
    assert "map_submap" in re.search(r"^SIDE := (.*)$", makefile, flags=re.M).group(1).split()
    assert makefile.count("vgicp_submap_plan.h") >= 2 and "vgicp_capi_map_submap.inl" in makefile


def test_module_exports_none_of_it_and_its_list_is_the_main_headers():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert not set(capi.MAP_SUBMAP_EXPORTS) & exported and lib.vgicp_abi_version() == 6
    assert exported == set(capi.EXPORTS + capi.MAP_POINTS_EXPORTS + capi.BATCH_EXPORTS + capi.EVALUATE_EXPORTS)
    main = open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()
    assert "scan_from_map" not in main and "vgicp_hip_map_submap" not in main


def test_struct_layouts_match_the_header(tmp_path):
    structs = (("vgicp_submap_params", capi.SubmapParams, PARAMS_FIELDS, [176, 0, 24, 32, 160, 168, 172]),
               ("vgicp_submap_stats", capi.SubmapStats, STATS_FIELDS, [56, 0, 8, 16, 24, 32, 36, 40, 48]))
    body = ""
    for name, mirror, fields, _ in structs:
        assert [f for f, _ in mirror._fields_] == list(fields)
        body += f'  printf("%zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {f}));\n' for f in fields)
        body += '  printf("\\n");\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_map_submap.h"\nint main(void) {\n' + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for line, (name, mirror, fields, want) in zip(lines, structs):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want, name


def test_the_entry_points_refuse_null_and_foreign_contexts_and_write_nothing():
    lib = capi.load_library()
    params = capi.SubmapParams((C.c_double * 3)(0.0, 0.0, 0.0), 1.0, (C.c_double * 16)(*np.eye(4).reshape(16)), 0, 0, 0)
    stats = capi.SubmapStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    before = bytes(stats)
    foreign, other = C.create_string_buffer(4096), C.create_string_buffer(4096)       # blocks that no build of the module stamped
    f, o = C.cast(foreign, C.c_void_p), C.cast(other, C.c_void_p)
    for dst, src, p in ((None, f, params), (f, None, params), (f, o, None), (f, o, params), (None, None, None)):
        rc = lib.vgicp_scan_from_map(dst, src, C.byref(p) if p is not None else None, C.byref(stats))
        assert rc == capi.ERR_BAD_ARGUMENT
        text = lib.vgicp_last_error(None).decode()
        assert ("not from one build" in text) if (dst and src and p is not None) else ("NULL pointer" in text)
    w = C.c_size_t(77)
    keys = (C.c_int32 * 3)(5, 5, 5)
    assert lib.vgicp_scan_from_map_keys(None, 1, keys, None, C.byref(w)) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_scan_from_map_keys(f, 1, keys, None, C.byref(w)) == capi.ERR_BAD_ARGUMENT
    assert "not from one build" in lib.vgicp_last_error(None).decode()
    assert bytes(stats) == before and w.value == 77 and list(keys) == [5, 5, 5]
    assert foreign.raw == bytes(4096) and other.raw == bytes(4096)


# ---- the host plan ----------------------------------------------------------------------------------------------------
def test_plan_submap_refuses_in_the_headers_order(tmp_path):
    """tests/native/submap_plan.cpp: the first rule that applies, over every combination of the facts."""
    out = native(tmp_path, "submap_plan", os.path.join(ROOT, "eskf_lio_amd", "csrc")).strip()
    assert out.startswith("ok ") and "MISMATCH" not in out, out
    counts = [int(v) for v in re.findall(r"rule \d+ (\d+)", out)]
    assert len(counts) == 11 and all(c > 0 for c in counts), out          # every rule is reached
    assert int(re.search(r"passed (\d+)", out).group(1)) > 0
    plan = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "vgicp_submap_plan.h")).read()
    inl = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "vgicp_capi_map_submap.inl")).read()
    assert "kLevelNotAskedText" in plan and inl.count("plan_submap(f)") == 2 and "several_devices(dst) || several_devices(src)" in inl


# ---- the shim ----------------------------------------------------------------------------------------------------------
def test_the_shim_carries_the_new_methods_and_the_weak_pragmas():
    lm = open(os.path.join(ROOT, "include", "eskf_lio_shim", "LocalMap.hpp")).read()
    icp = open(os.path.join(ROOT, "include", "eskf_lio_shim", "Registration.hpp")).read()
    for name in ("#pragma weak vgicp_scan_from_map\n", "#pragma weak vgicp_scan_from_map_keys\n", "SubmapStats scanFromMap(",
                 "const LocalMap & source, const Vector3d & center, double radius, const Isometry3d & frame, size_t minCount = 0,",
                 "int level = 0)", "libvgicp_hip_map_submap.so", '#include "../vgicp_hip_map_submap.h"'):
        assert name in lm, name
    for name in ("Isometry3d alignSubmap(", "LocalMap & source, LocalMap & target, const Isometry3d & anchor, double radius, const Isometry3d & guess",
                 "target.scanFromMap(source, anchor.translation(), radius, anchor.inverse(), minCount, level)",
                 "chainResidentScan(ctx, guess, schedule_)", "lastSubmap()"):
        assert name in icp, name


def test_the_shim_compiles_over_the_stand_in_types(tmp_path):
    """The shim's headers with the new methods, without Eigen (ShimTypes.hpp's stand-ins), under -Werror."""
    src = tmp_path / "weak.cpp"
    src.write_text('#include "eskf_lio_shim/Registration.hpp"\n'
                   'int main() { return (vgicp_scan_from_map == nullptr && vgicp_scan_from_map_keys == nullptr) ? 0 : 1; }\n')
    cmd = ["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-Wno-address", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "native"), "-fsyntax-only", str(src)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


# ---- the rule: the restatement on hand-worked cases -------------------------------------------------------------------------
H = 0.5


def one_voxel(key, count=1):
    keys = np.array([key], dtype=np.int32)
    means = (keys + 0.5) * H
    covs = np.array([[1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 3.0]]) * 0.01
    return keys, means, covs, np.array([count], dtype=np.uint64)


def test_a_voxel_at_exactly_the_radius_is_kept_and_one_ulp_beyond_is_dropped():
    center = (0.25, 0.25, 0.25)                      # the centre of voxel (0, 0, 0)
    for key, radius in (((3, 4, 0), 2.5), ((0, 0, -5), 2.5), ((2, 3, 6), 3.5), ((1, 0, 0), 0.5), ((0, 0, 0), 0.0)):
        v = one_voxel(key)
        assert not ms.too_far(v[0], H, center, radius)[0]
        assert len(ms.submap(*v, H, center, radius)) == 1
        below = np.nextafter(radius, -math.inf)
        if radius > 0.0:
            assert ms.too_far(v[0], H, center, below)[0]          # the radius one ulp short: the voxel one ulp beyond it
            s = ms.submap(*v, H, center, below)
            assert (len(s), s.voxels, s.too_far, s.too_few) == (0, 1, 1, 0)
    assert len(ms.submap(*one_voxel((1000000, -1000000, 7)), H, center, math.inf)) == 1
    # eviction's own arithmetic: ((double)k + 0.5) * h - c, squares summed left to right
    k = np.array([[7, -3, 2]], dtype=np.int32)
    c = np.array([0.1, 0.2, 0.3])
    d = (k[0].astype(np.float64) + 0.5) * 0.3 - c
    r = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    assert not ms.too_far(k, 0.3, c, r)[0] and ms.too_far(k, 0.3, c, np.nextafter(r, 0.0))[0]


def test_min_count_zero_and_one_select_every_voxel_and_two_asks_for_two():
    center = (0.25, 0.25, 0.25)
    for count in (1, 2):
        for min_count, kept in ((0, True), (1, True), (2, count >= 2)):
            s = ms.submap(*one_voxel((1, 1, 1), count), H, center, math.inf, None, min_count)
            assert (len(s) == 1) == kept and s.too_few == (0 if kept else 1) and s.too_far == 0, (count, min_count)
    far = ms.submap(*one_voxel((9, 9, 9), 1), H, center, 1.0, None, 2)          # beyond the radius: too far, not too few
    assert (len(far), far.too_far, far.too_few) == (0, 1, 0)


def test_the_identity_frame_returns_the_input_bits():
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(-20, 20, size=(300, 3)), axis=0).astype(np.int32)
    means = (keys + rng.uniform(0.0, 1.0, size=keys.shape)) * 0.3
    covs = synth.disc_covariances(6, 16, np.arange(len(keys), dtype=np.uint64))
    counts = rng.integers(1, 9, size=len(keys)).astype(np.uint64)
    s = ms.submap(keys, means, covs, counts, 0.3, (0.0, 0.0, 0.0), math.inf)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    assert np.array_equal(s.keys, keys[order]) and np.array_equal(s.counts, counts[order])
    assert s.points.tobytes() == means[order].tobytes() and s.covs.tobytes() == covs[order].tobytes()
    assert (s.voxels, s.too_far, s.too_few) == (len(keys), 0, 0)


def test_a_quarter_turn_permutes_the_covariance_exactly():
    """R = 90 degrees about z: x -> y, y -> -x.  R C R^T has the entries of C, moved and signed, with no rounding."""
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (4.0, 8.0, -2.0)
    rng = np.random.default_rng(8)
    means = rng.uniform(-5.0, 5.0, size=(50, 3))
    A = rng.normal(size=(50, 3, 3))
    Cm = A @ A.transpose(0, 2, 1)                                    # C[n, r, c], symmetric up to rounding
    covs = np.ascontiguousarray(Cm.transpose(0, 2, 1).reshape(50, 9))          # column-major
    pts, rot = ms.transform(means, covs, T)
    assert np.array_equal(pts, np.stack([-means[:, 1] + 4.0, means[:, 0] + 8.0, means[:, 2] - 2.0], axis=1))
    Rm = rot.reshape(50, 3, 3).transpose(0, 2, 1)
    perm, sign = [1, 0, 2], np.array([-1.0, 1.0, 1.0])               # row r of R C R^T is row perm[r] of C, signed
    want = np.empty_like(Cm)
    for r in range(3):
        for c in range(3):
            want[:, r, c] = sign[r] * sign[c] * Cm[:, perm[r], perm[c]]
    assert np.array_equal(Rm, want)
    # ... and against the generator's conjugation, which sums in the same order
    assert np.array_equal(rot, synth._conjugate(T[:3, :3], covs))


# ---- the purpose, on the oracle alone -----------------------------------------------------------------------------------
def test_the_oracle_meets_the_basin_condition_on_the_end_to_end_recipe(oracle):
    """What tests/test_map_submap.py asks of the device, met by the CPU oracle alone on the same inputs: B's submap around
    the anchor registers on A to within half a voxel, and closer than the guess was (measured: 9.4 mm from 197.7 mm)."""
    a_frames, b_frames, D, anchor = ms.two_sessions(oracle)
    A, B = oracle.OracleMap(ms.VOXEL, ms.CAP), oracle.OracleMap(ms.VOXEL, ms.CAP)
    for omap, frames in ((A, a_frames), (B, b_frames)):
        for p, c, pose in frames:
            omap.insert(*oracle.transform(p, c, pose))
    sub = ms.submap(*B.export(), ms.VOXEL, anchor[:3, 3], ms.RADIUS, synth.invert_pose(anchor), ms.MIN_COUNT)
    assert len(sub) > 1000 and sub.too_far > 0 and sub.too_few > 0
    got = A.align(sub.points, sub.covs, anchor, ms.ALIGN["max_iteration"], ms.ALIGN["translation_sq_threshold"], ms.ALIGN["cosine_threshold"])
    error, guess_error = ms.anchor_error(got.pose, D, anchor), ms.anchor_error(anchor, D, anchor)
    print(f"oracle: {len(sub)} points, {got.iterations} rounds, anchor error {1e3 * error:.2f} mm from a guess {1e3 * guess_error:.1f} mm off")
    assert got.converged and error < ms.VOXEL / 2 and error < guess_error
    assert 0.15 < guess_error < ms.VOXEL
