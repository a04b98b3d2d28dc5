"""Map merge (include/vgicp_hip_map_merge.h) without a device: the header against the Python mirror, the Makefile and the
libraries' exports, the struct layouts, the host plan (plan_merge's refusals in their order, the growth, the scratch), the
shim's mergeFrom, and the numpy restatement of the rule — pinned against the oracle's insertion where every count is one,
and checked for the properties the header states."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import map_merge_reference as mm
from eskf_lio_amd import capi, synth
from test_evaluate_cpu import declared
from test_map_gated_cpu import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS_FIELDS = ("center", "radius", "frame", "min_count", "max_count", "reserved")
STATS_FIELDS = ("voxels", "selected", "too_far", "too_few", "created", "updated", "frozen", "points", "launches", "reserved", "seconds",
                "device_seconds")
H = 0.5


# ---- header, mirror, Makefile and libraries ------------------------------------------------------------------------------
def test_header_mirror_makefile_and_library_agree():
    lib = capi.load_library()
    assert declared("vgicp_hip_map_merge.h") == sorted(capi.MAP_MERGE_EXPORTS) == ["vgicp_map_merge"]
    assert capi.SIDE_EXPORTS["map_merge"] is capi.MAP_MERGE_EXPORTS
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_merge.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_map_merge.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("map_merge")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.MAP_MERGE_EXPORTS)
    assert all(hasattr(lib, name) for name in capi.MAP_MERGE_EXPORTS)
    assert re.findall(r"^ \*\s+(\d+)\. ", text, flags=re.M) == [str(k) for k in range(1, 14)]          # the thirteen refusals
    makefile = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "Makefile")).read()
    side = re.search(r"^SIDE := (.*)$", makefile, flags=re.M).group(1).split()
    assert "map_merge" in side and sorted(side) == sorted(capi.SIDE_EXPORTS)
    parts = re.search(r"^CAPI_PARTS := ((?:.*\\\n)*.*)$", makefile, flags=re.M).group(1)
    headers = re.search(r"^CONTEXT_HEADERS := ((?:.*\\\n)*.*)$", makefile, flags=re.M).group(1)
    assert "vgicp_capi_map_merge.inl" in parts.split() and "vgicp_merge_plan.h" in headers.split()
    assert "$(SIDE:%=../../include/vgicp_hip_%.h)" in headers


def test_module_exports_none_of_it_and_its_list_is_the_main_headers():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert not set(capi.MAP_MERGE_EXPORTS) & exported and lib.vgicp_abi_version() == 6
    assert exported == set(capi.EXPORTS + capi.MAP_POINTS_EXPORTS + capi.BATCH_EXPORTS + capi.EVALUATE_EXPORTS)
    main = open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()
    assert "map_merge" not in main


def test_struct_layouts_match_the_header(tmp_path):
    structs = (("vgicp_merge_params", capi.MergeParams, PARAMS_FIELDS, [184, 0, 24, 32, 160, 168, 176]),
               ("vgicp_merge_stats", capi.MergeStats, STATS_FIELDS, [88, 0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 80]))
    body = ""
    for name, mirror, fields, _ in structs:
        assert [f for f, _ in mirror._fields_] == list(fields)
        body += f'  printf("%zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {f}));\n' for f in fields)
        body += '  printf("\\n");\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_map_merge.h"\nint main(void) {\n' + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for line, (name, mirror, fields, want) in zip(lines, structs):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want, name
    assert C.sizeof(capi.MergeParams) == 184 and C.sizeof(capi.MergeStats) == 88


def test_the_entry_point_refuses_null_and_foreign_contexts_and_writes_nothing():
    lib = capi.load_library()
    params = capi.MergeParams((C.c_double * 3)(0.0, 0.0, 0.0), 1.0, (C.c_double * 16)(*np.eye(4).reshape(16)), 0, 0, 0)
    stats = capi.MergeStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    before = bytes(stats)
    foreign, other = C.create_string_buffer(4096), C.create_string_buffer(4096)       # blocks that no build of the module stamped
    f, o = C.cast(foreign, C.c_void_p), C.cast(other, C.c_void_p)
    for dst, src, p in ((None, f, params), (f, None, params), (f, o, None), (f, o, params), (f, f, params), (None, None, None)):
        rc = lib.vgicp_map_merge(dst, src, C.byref(p) if p is not None else None, C.byref(stats))
        assert rc == capi.ERR_BAD_ARGUMENT
        text = lib.vgicp_last_error(None).decode()
        assert ("not from one build" in text) if (dst and src and p is not None) else ("NULL pointer" in text)
    assert bytes(stats) == before and foreign.raw == bytes(4096) and other.raw == bytes(4096)


# ---- the host plan ----------------------------------------------------------------------------------------------------
def test_plan_merge_refuses_in_the_headers_order(tmp_path):
    """tests/native/merge_plan.cpp: the first rule that applies, over every combination of the facts; the growth is the
    insertion's; the scratch's pieces do not overlap."""
    out = native(tmp_path, "merge_plan", os.path.join(ROOT, "eskf_lio_amd", "csrc")).strip()
    assert out.startswith("ok ") and "MISMATCH" not in out, out
    counts = [int(v) for v in re.findall(r"rule \d+ (\d+)", out)]
    assert len(counts) == 13 and all(c > 0 for c in counts), out          # every rule is reached
    assert int(re.search(r"passed (\d+)", out).group(1)) > 0
    # the same program under the address and undefined-behaviour sanitizers: stand-alone, host code only
    exe = tmp_path / "merge_plan_sanitized"
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "merge_plan.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == out, run.stdout[-1000:] + run.stderr[-2000:]
    inl = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "vgicp_capi_map_merge.inl")).read()
    assert inl.count("plan_merge(f)") == 2 and "several_devices(dst) || several_devices(src)" in inl
    assert "ensure_table(dst, upper)" in inl and "begin_map_update(dst)" in inl and inl.count("hipStreamSynchronize") == 1


# ---- the shim ----------------------------------------------------------------------------------------------------------
def test_the_shims_merge_from_forwards_and_refuses(tmp_path):
    """tests/native/shim_merge.cpp against a stand-in of the C ABI, with and without the entry point."""
    lm = open(os.path.join(ROOT, "include", "eskf_lio_shim", "LocalMap.hpp")).read()
    for name in ("#pragma weak vgicp_map_merge\n", "MergeStats mergeFrom(", "libvgicp_hip_map_merge.so", '#include "../vgicp_hip_map_merge.h"',
                 "const LocalMap & source, const Isometry3d & frame, const Vector3d & center, double radius, size_t minCount = 0,",
                 "size_t maxCount = 0)"):
        assert name in lm, name
    for flags, last in (((), "ok with the library"), (("-DWITHOUT_MERGE_LIBRARY",), "ok without the library")):
        exe = tmp_path / ("shim_merge" + str(len(flags)))
        cmd = ["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-Wno-address", *flags, "-I" + os.path.join(ROOT, "include"),
               "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_merge.cpp")]
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-3000:]
        run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == last, run.stdout[-2000:] + run.stderr[-1000:]
    # no existing method's route has changed
    assert "mergeFrom" not in open(os.path.join(ROOT, "tests", "golden", "shim_routes.txt")).read()


# ---- the reference, pinned against the oracle ------------------------------------------------------------------------------
EMPTY = (np.zeros((0, 3), np.int32), np.zeros((0, 3)), np.zeros((0, 9)), np.zeros(0, np.uint64))


def crowd(n, seed, span=3.0):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-span, span, size=(n, 3))
    covs = synth.disc_covariances(seed + 1, 16, np.arange(n, dtype=np.uint64))
    return pts, covs


@pytest.mark.parametrize("cap", (1, 3, 1000))
def test_with_every_count_one_the_fold_is_the_oracles_insertion(oracle, cap):
    """Voxel(max, p, C) and Voxel::addPoint in the order of the points, two batches: the second finds records."""
    omap = oracle.OracleMap(H, cap)
    state = EMPTY
    for batch, n in enumerate((3000, 2000)):
        pts, covs = crowd(n, 10 + batch)
        omap.insert(pts, covs)
        got = mm.merge(state, pts, covs, np.ones(n, dtype=np.uint64), H, cap)
        assert np.array_equal(mm.voxel_keys(pts, H), oracle.voxel_index(H, pts))
        assert mm.exports_equal(got.export(), omap.export())          # ==, counts included
        assert got.points + got.frozen == n and (got.frozen > 0) == (cap < 1000)
        assert (got.updated > 0) == (batch == 1 and cap > 1)
        state = got.export()
    assert int(state[3].max()) == min(cap, int(state[3].max())) and len(state[0]) > 500


# ---- the reference's properties ------------------------------------------------------------------------------------------------
def voxel(key, count, seed):
    rng = np.random.default_rng(seed)
    mean = (np.asarray(key, dtype=np.float64) + rng.uniform(0.1, 0.9, size=3)) * H
    A = rng.normal(size=(3, 3))
    return mean, (A @ A.T * 0.01).T.reshape(9), count


def test_a_single_contributor_comes_through_verbatim():
    m, c, n = voxel((2, -3, 1), 40, 1)
    got = mm.merge(EMPTY, [m], [c], [n], H)
    assert np.array_equal(got.keys, [[2, -3, 1]]) and got.counts[0] == 40
    assert got.means.tobytes() == m.tobytes() and got.covs.tobytes() == c.tobytes()
    assert (got.created, got.updated, got.frozen, got.points) == (1, 0, 0, 40)
    # ... under a cap too: a fresh voxel always accepts its first contributor, whatever its count
    capped = mm.merge(EMPTY, [m], [c], [n], H, max_count=5)
    assert capped.counts[0] == 40 and capped.frozen == 0 and capped.means.tobytes() == m.tobytes()


def test_a_frozen_voxel_is_untouched_and_counts_what_it_refused():
    m, c, n = voxel((0, 0, 0), 6, 2)
    dst = (np.array([[0, 0, 0]], np.int32), m[None], c[None], np.array([n], np.uint64))
    others = [voxel((0, 0, 0), k, 3 + k) for k in (1, 9)]
    got = mm.merge(dst, [o[0] for o in others], [o[1] for o in others], [o[2] for o in others], H, max_count=6)
    assert (got.created, got.updated, got.frozen, got.points) == (0, 0, 2, 0)
    assert got.means.tobytes() == m.tobytes() and got.covs.tobytes() == c.tobytes() and got.counts[0] == 6
    # one below the cap: the first is accepted whole (the count passes the cap), the second is frozen out
    got = mm.merge(dst, [o[0] for o in others], [o[1] for o in others], [o[2] for o in others], H, max_count=7)
    assert (got.updated, got.frozen, got.points, int(got.counts[0])) == (1, 1, 1, 7)
    got = mm.merge(dst, [o[0] for o in others][::-1], [o[1] for o in others][::-1], [o[2] for o in others][::-1], H, max_count=7)
    assert (got.updated, got.frozen, got.points, int(got.counts[0])) == (1, 1, 9, 15)


def test_the_counts_are_conserved_and_the_mean_is_the_weighted_mean():
    rng = np.random.default_rng(7)
    keys = np.unique(rng.integers(-3, 3, size=(150, 3)), axis=0).astype(np.int32)
    dst = (keys, (keys + rng.uniform(0.1, 0.9, size=keys.shape)) * H, synth.disc_covariances(8, 16, np.arange(len(keys), dtype=np.uint64)),
           rng.integers(1, 30, size=len(keys)).astype(np.uint64))
    n = 600
    pts, covs = crowd(n, 9, span=2.5)
    counts = rng.integers(1, 50, size=n).astype(np.uint64)
    for cap in (0, 25):
        got = mm.merge(dst, pts, covs, counts, H, cap)
        assert int(got.counts.sum()) - int(dst[3].sum()) == got.points          # integers: exact
        assert got.points + 0 <= int(counts.sum()) and (got.frozen > 0) == (cap != 0)
        assert len(got.keys) == len(keys) + got.created and got.created > 20 and got.updated > 20
    # without a cap the mean of a voxel is the count-weighted mean of everything that went in, to rounding
    got = mm.merge(dst, pts, covs, counts, H)
    pk = mm.voxel_keys(pts, H)
    for j in (0, len(got.keys) // 2, len(got.keys) - 1):
        key = got.keys[j]
        inside = (pk == key).all(axis=1)
        was = (dst[0] == key).all(axis=1)
        w = np.concatenate([dst[3][was], counts[inside]]).astype(np.float64)
        x = np.concatenate([dst[1][was], pts[inside]])
        assert np.allclose(got.means[j], (w[:, None] * x).sum(axis=0) / w.sum(), rtol=1e-12, atol=1e-12)
        assert got.counts[j] == int(w.sum())


def test_the_order_of_two_contributors_shows_in_the_bits():
    """The fold is left to right and every step rounds: a record that takes b and then c is not, in general, the record
    that takes c and then b.  (Two contributors to a FRESH voxel do commute: nn * a + cc * b is one commutative sum.)
    Over 300 drawn cases at least one differs in a bit — the ORDER clause says something."""
    differ = 0
    for seed in range(300):
        a, b, c = (voxel((1, 1, 1), k, 10 * seed + k) for k in (3, 5, 7))
        dst = (np.array([[1, 1, 1]], np.int32), a[0][None], a[1][None], np.array([a[2]], np.uint64))
        ab = mm.merge(dst, [b[0], c[0]], [b[1], c[1]], [b[2], c[2]], H)
        ba = mm.merge(dst, [c[0], b[0]], [c[1], b[1]], [c[2], b[2]], H)
        fresh = (mm.merge(EMPTY, [b[0], c[0]], [b[1], c[1]], [b[2], c[2]], H), mm.merge(EMPTY, [c[0], b[0]], [c[1], b[1]], [c[2], b[2]], H))
        assert fresh[0].means.tobytes() == fresh[1].means.tobytes() and fresh[0].covs.tobytes() == fresh[1].covs.tobytes()
        assert ab.counts[0] == ba.counts[0] == 15
        assert np.allclose(ab.means, ba.means, rtol=1e-14) and np.allclose(ab.covs, ba.covs, rtol=1e-12, atol=1e-18)
        differ += ab.means.tobytes() != ba.means.tobytes() or ab.covs.tobytes() != ba.covs.tobytes()
    assert differ >= 1
    print(f"{differ} of 300 swapped pairs differ in at least one bit")


def test_select_and_move_is_the_submaps_selection_and_transform():
    import map_submap_reference as ms
    rng = np.random.default_rng(11)
    keys = np.unique(rng.integers(-6, 6, size=(400, 3)), axis=0).astype(np.int32)
    means = (keys + rng.uniform(0.1, 0.9, size=keys.shape)) * H
    covs = synth.disc_covariances(12, 16, np.arange(len(keys), dtype=np.uint64))
    counts = rng.integers(1, 6, size=len(keys)).astype(np.uint64)
    T = np.eye(4)
    a = np.deg2rad(25.0)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (0.5, -1.0, 0.25)
    pts, rot, cnt, four = mm.select_and_move((keys, means, covs, counts), H, (0.25, 0.25, 0.25), 2.0, T, 2)
    want = ms.submap(keys, means, covs, counts, H, (0.25, 0.25, 0.25), 2.0, T, 2)
    assert four == (want.voxels, len(want), want.too_far, want.too_few) and len(want) > 20
    assert sorted(map(bytes, pts)) == sorted(map(bytes, want.points)) and sorted(map(bytes, rot)) == sorted(map(bytes, want.covs))
    assert math.isclose(float(cnt.sum()), float(want.counts.sum()))
