"""Locate (include/vgicp_hip_map_locate.h) without a device: the header against the Python mirror, the libraries' exports,
the struct layouts, the host plan (plan_locate's refusals in their order), the shim over a stubbed ABI, the numpy
restatement of the rule against a brute force and against properties of its own, and the point of it all on the oracle:
from guesses metres and tens of degrees off, locate and the coarse-to-fine chain end where the plain align from the
identity ends."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_levels_reference as ml
import map_locate_reference as lo
from eskf_lio_amd import capi
from test_evaluate_cpu import declared
from test_map_gated_cpu import native
from test_map_levels_cpu import straddling_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS_FIELDS = ("level", "window", "stride")
BEST_FIELDS = ("hits", "cell", "offset", "points", "skipped", "reserved", "pose")
STATS_FIELDS = ("cells", "launches", "seconds", "device_seconds")


# ---- header and libraries ---------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_function_and_the_library_exports_it():
    lib = capi.load_library()
    assert declared("vgicp_hip_map_locate.h") == sorted(capi.MAP_LOCATE_EXPORTS) == ["vgicp_locate_resident"]
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_locate.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_map_locate.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    for name, value, mirror in (("VGICP_LOCATE_MAX_POSES", capi.LOCATE_MAX_POSES, lo.MAX_POSES),
                                ("VGICP_LOCATE_MAX_HALF_WIDTH", capi.LOCATE_MAX_HALF_WIDTH, lo.MAX_HALF_WIDTH),
                                ("VGICP_LOCATE_MAX_CELLS", capi.LOCATE_MAX_CELLS, lo.MAX_CELLS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text) and value == mirror, name
    assert (capi.LOCATE_MAX_POSES, capi.LOCATE_MAX_HALF_WIDTH, capi.LOCATE_MAX_CELLS) == (64, 32, 4096)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("map_locate")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.MAP_LOCATE_EXPORTS)
    assert hasattr(lib, "vgicp_locate_resident")
    assert re.findall(r"^ \*   (\d)\. ", text, flags=re.M) == [str(k) for k in range(1, 7)]


def test_module_exports_none_of_it_and_its_list_is_the_main_headers():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert not set(capi.MAP_LOCATE_EXPORTS) & exported and lib.vgicp_abi_version() == 6
    assert "locate" not in " ".join(sorted(exported))
    main = open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()
    assert "vgicp_locate" not in main and "vgicp_hip_map_locate" not in main


def test_struct_layouts_match_the_header(tmp_path):
    structs = (("vgicp_locate_params", capi.LocateParams, PARAMS_FIELDS, [20, 0, 4, 16]),
               ("vgicp_locate_best", capi.LocateBest, BEST_FIELDS, [160, 0, 4, 8, 20, 24, 28, 32]),
               ("vgicp_locate_stats", capi.LocateStats, STATS_FIELDS, [24, 0, 4, 8, 16]))
    body = ""
    for name, mirror, fields, _ in structs:
        assert [f for f, _ in mirror._fields_] == list(fields)
        body += f'  printf("%zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {f}));\n' for f in fields)
        body += '  printf("\\n");\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_map_locate.h"\nint main(void) {\n' + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for line, (name, mirror, fields, want) in zip(lines, structs):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want, name


def test_the_entry_point_refuses_a_null_context_and_a_foreign_one_and_writes_nothing():
    lib = capi.load_library()
    poses = (C.c_double * 16)(*np.eye(4).reshape(16))
    params = capi.LocateParams(0, (C.c_int32 * 3)(1, 1, 1), 1)
    best = (capi.LocateBest * 1)()
    stats = capi.LocateStats()
    hits = (C.c_uint32 * 27)(*([7] * 27))
    C.memset(best, 0xA5, C.sizeof(best))
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    before = bytes(best), bytes(stats)
    foreign = C.create_string_buffer(4096)       # a block that no build of the module stamped
    for ctx in (None, C.cast(foreign, C.c_void_p)):
        assert lib.vgicp_locate_resident(ctx, poses, 1, C.byref(params), best, hits, C.byref(stats)) == capi.ERR_BAD_ARGUMENT
        if ctx is not None:
            assert "not from one build" in lib.vgicp_last_error(None).decode()
    assert (bytes(best), bytes(stats)) == before and list(hits) == [7] * 27
    assert foreign.raw == bytes(4096)


# ---- the host plan ----------------------------------------------------------------------------------------------------
def test_plan_locate_refuses_in_the_headers_order(tmp_path):
    """tests/native/locate_plan.cpp: the first rule that applies, over every combination of the facts."""
    out = native(tmp_path, "locate_plan", os.path.join(ROOT, "eskf_lio_amd", "csrc")).strip()
    assert out.startswith("ok ") and "MISMATCH" not in out, out
    counts = [int(v) for v in re.findall(r"rule \d (\d+)", out)]
    assert len(counts) == 6 and all(c > 0 for c in counts), out          # every rule is reached
    assert int(re.search(r"passed (\d+)", out).group(1)) > 0


# ---- the shim ----------------------------------------------------------------------------------------------------------
def test_shim_locate_over_a_stubbed_abi(tmp_path):
    """tests/native/shim_locate.cpp: ICP::yawFan / setLocate / locate against a stand-in of the C ABI that records the
    calls (tests/golden/shim_routes.txt, held by tests/test_capi_cpu.py, is unchanged)."""
    exe = tmp_path / "shim_locate"
    cmd = ["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_locate.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout[-1000:] + run.stderr[-500:]
    icp = open(os.path.join(ROOT, "include", "eskf_lio_shim", "Registration.hpp")).read()
    for name in ("yawFan(", "void setLocate(", "Isometry3d locate(", "lastLocation()", "#pragma weak vgicp_locate_resident",
                 'reg["locate"]', 'loc["window"]', "libvgicp_hip_map_locate.so"):
        assert name in icp, name


# ---- the rule: the restatement against a brute force and its own properties -----------------------------------------------
@pytest.fixture(scope="module")
def small():
    """A map with keys on both sides of 0 in every axis, its level 1, and points among them."""
    keys, means, covs, counts = straddling_map()
    levels = ml.levels_of(keys, means, covs, counts, 1)
    rng = np.random.default_rng(11)
    pts = rng.uniform(-1.9, 1.9, size=(90, 3))
    return levels, pts


@pytest.mark.parametrize("level", (0, 1))
def test_the_restatement_is_the_plain_triple_loop(small, level):
    levels, pts = small
    keys, h = levels[level].keys, ml.VOXEL * 2 ** level
    assert (keys.min(axis=0) < 0).all() and (keys.max(axis=0) > 0).all()
    total = 0
    for T in (np.eye(4), lo.wrong_guess((0.31, -0.22, 0.13), 25.0)):
        for window, stride in (((0, 0, 0), 1), ((2, 1, 0), 1), ((1, 2, 3), 3), ((0, 0, 2), 89)):
            want = lo.brute_force(keys, h, pts, T, window, stride)
            got, points, skipped = lo.score(lo.KeySet(keys), h, pts, T, window, stride)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (level, window, stride)
            assert points == -(-len(pts) // stride) and skipped == 0
            total += int(want.sum())
    assert total > 100


def test_a_point_without_a_key_is_skipped_and_counted(small):
    levels, pts = small
    keys = lo.KeySet(levels[0].keys)
    odd = pts[:8].copy()
    odd[1, 0] = np.nan
    odd[2, 1] = np.inf
    odd[3, 2] = (2.0 ** 30 + 2.0) * ml.VOXEL          # a key beyond 2^30
    odd[4, 2] = 2.0 ** 30 * ml.VOXEL                  # at the edge, within a rounding of 2^30: still defined
    hits, points, skipped = lo.score(keys, ml.VOXEL, odd, np.eye(4), (1, 1, 1))
    assert (points, skipped) == (5, 3)
    assert np.array_equal(hits, lo.score(keys, ml.VOXEL, odd[[0, 4, 5, 6, 7]], np.eye(4), (1, 1, 1))[0])
    assert lo.score(keys, ml.VOXEL, odd, np.eye(4), (1, 1, 1), stride=2)[1:] == (3, 1)          # points 0, 4, 6 and the skipped 2


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_a_one_axis_window_moves_exactly_its_own_index(small, axis):
    """Window (5, 0, 0), (0, 5, 0) and (0, 0, 5): cell c is the shift c - 5 along that axis and no other."""
    levels, pts = small
    keys = lo.KeySet(levels[0].keys)
    window = [0, 0, 0]
    window[axis] = 5
    d = lo.cells_of(window)
    assert len(d) == 11 and np.array_equal(d[:, axis], np.arange(-5, 6)) and not np.delete(d, axis, axis=1).any()
    hits = lo.score(keys, ml.VOXEL, pts, np.eye(4), window)[0]
    for c in range(11):
        shifted_keys = levels[0].keys.astype(np.int64).copy()
        shifted_keys[:, axis] -= c - 5          # the map moved the other way, exactly
        assert hits[c] == lo.score(lo.KeySet(shifted_keys), ml.VOXEL, pts, np.eye(4), (0, 0, 0))[0][0], (axis, c)
    # and the full index: dx fastest, dz slowest
    d = lo.cells_of((2, 1, 3))
    for c, (dx, dy, dz) in enumerate(d):
        assert c == ((dz + 3) * 3 + (dy + 1)) * 5 + (dx + 2)


def test_the_best_cell_is_the_lowest_index_among_ties():
    """Two equal peaks: the same cluster of voxels twice, 3 voxels apart along x; the points sit in the gap's middle."""
    cluster = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.int64)
    keys = np.concatenate([cluster + (-3, 0, 0), cluster + (3, 0, 0)])
    pts = (cluster + 0.5) * ml.VOXEL
    bests, plane = lo.locate(keys, ml.VOXEL, pts, [np.eye(4)], (4, 1, 1))
    cells = lo.cells_of((4, 1, 1))
    peaks = np.flatnonzero(plane[0] == plane[0].max())
    assert plane[0].max() == 4 and [tuple(cells[c]) for c in peaks] == [(-3, 0, 0), (3, 0, 0)]
    b = bests[0]
    assert b.cell == peaks[0] and b.offset == (-3, 0, 0) and b.hits == 4 and (b.points, b.skipped) == (4, 0)
    assert b.pose[0, 3] == -3.0 * ml.VOXEL and b.pose[1, 3] == 0.0 and np.array_equal(b.pose[:3, :3], np.eye(3))
    # an empty map: all zero, the best cell is cell 0
    bests, plane = lo.locate(np.zeros((0, 3), dtype=np.int32), ml.VOXEL, pts, [np.eye(4)], (4, 1, 1))
    assert not plane.any() and bests[0].cell == 0 and bests[0].offset == (-4, -1, -1) and bests[0].hits == 0


def test_on_a_dyadic_grid_a_shift_of_the_key_is_a_translation_of_the_pose():
    """Voxel size 0.25, points and translations on a grid of 2^-6: every sum is exact, so hits(pose, d) equals
    hits(pose translated by d h, window 0), met with ==."""
    rng = np.random.default_rng(3)
    h = 0.25
    keys = lo.KeySet(np.unique(rng.integers(-8, 8, size=(700, 3)), axis=0))
    pts = rng.integers(-128, 128, size=(300, 3)) / 64.0
    T = np.eye(4)
    T[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = (3 / 64.0, -17 / 64.0, 5 / 64.0)
    window = (3, 2, 1)
    hits = lo.score(keys, h, pts, T, window)[0]
    for c, d in enumerate(lo.cells_of(window)):
        moved = np.array(T)
        moved[:3, 3] += d * h
        assert hits[c] == lo.score(keys, h, pts, moved, (0, 0, 0))[0][0], d
    assert hits.max() > 20 and hits.min() < hits.max()


# ---- the point of it --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def experiment(oracle):
    """The recipe of the coarse-to-fine experiment: levels 0 .. 3 as oracle maps and as key sets, the scan, P*."""
    mp, mc, sp, sc = ml.recipe(oracle)
    omap = oracle.OracleMap(ml.VOXEL, ml.CAP)
    omap.insert(mp, mc)
    levels = ml.levels_of(*omap.export(), 3)
    maps = [omap] + [ml.oracle_level_map(oracle, levels[l], ml.VOXEL * 2 ** l) for l in (1, 2, 3)]
    star = omap.align(sp, sc, np.eye(4), ml.FINE["max_iteration"], ml.FINE["translation_sq_threshold"], ml.FINE["cosine_threshold"])
    return maps, [lo.KeySet(lv.keys) for lv in levels], sp, sc, star.pose


@pytest.mark.parametrize("case", range(len(lo.WRONG_GUESSES)))
def test_locate_and_the_chain_end_at_p_star_from_guesses_the_chain_alone_fails_from(oracle, experiment, case):
    """Level 3, window (4, 4, 1), 64 yaws, keep 4, strides 1 and 4.  The limits are the levels test's, conditions stated in
    voxels, not tuned numbers.  Measured here: the chain from the wrong guess ends 6.91, 4.84 and 2.86 m from P*; the winner
    0.5 - 1.2 mm, with 1 656 - 1 670 level-0 matches against at most 1 357 for a candidate that ends far away."""
    maps, keysets, sp, sc, star = experiment
    guess = lo.wrong_guess(*lo.WRONG_GUESSES[case])
    if case < lo.CHAIN_CASES:
        pose, _ = ml.oracle_chain(oracle, maps, sp, sc, guess)
        far = ml.distance(pose, star)
        print(f"guess {lo.WRONG_GUESSES[case]}: the chain alone ends {far:.2f} m from P*")
        assert far >= ml.FAR_LIMIT
    for stride in lo.STRIDES:
        winner, found = lo.pipeline(oracle, maps, keysets, sp, sc, guess, stride=stride)
        ends = [ml.distance(c.pose, star) for c in found]
        near = ml.distance(winner.pose, star)
        print(f"guess {lo.WRONG_GUESSES[case]} stride {stride}: winner pose {winner.index} offset {winner.offset} {winner.hits} hits, "
              f"{1e3 * near:.3f} mm from P*, {winner.matches} matches; candidates "
              f"{[(c.index, c.hits, round(e, 3), c.matches) for c, e in zip(found, ends)]}")
        assert near <= ml.NEAR_LIMIT
        lost = [c.matches for c, e in zip(found, ends) if e >= ml.FAR_LIMIT]
        assert all(winner.matches > m for m in lost), (winner.matches, lost)
