"""Map levels (include/vgicp_hip_map_levels.h) without a device: the header against the Python mirror, the libraries'
exports, the host plan (plan_levels' refusals in their order), the numpy restatement of the rule against brute-force
properties, the key identity that lets a level be addressed by the map's own key function, and the point of it all on
the oracle: a coarse-to-fine chain converges from guesses the plain align fails from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_levels_reference as ml
from eskf_lio_amd import capi
from test_evaluate_cpu import declared
from test_map_gated_cpu import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = ["vgicp_align_resident_levels", "vgicp_map_level_export", "vgicp_map_level_size", "vgicp_map_levels_build"]
STATS_FIELDS = ("voxels", "slots", "levels", "launches", "seconds", "device_seconds")


# ---- header and libraries ---------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_four_functions_and_the_library_exports_them():
    lib = capi.load_library()
    assert declared("vgicp_hip_map_levels.h") == sorted(capi.MAP_LEVELS_EXPORTS) == LEVELS
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_levels.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_map_levels.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    assert re.search(r"#define\s+VGICP_LEVELS_MAX\s+%d\b" % capi.LEVELS_MAX, text) and ml.LEVELS_MAX == capi.LEVELS_MAX == 4
    assert re.search(r"#define\s+VGICP_LEVEL_STAGES_MAX\s+%d\b" % capi.LEVEL_STAGES_MAX, text)
    assert ml.LEVEL_STAGES_MAX == capi.LEVEL_STAGES_MAX == 8
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("map_levels")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.MAP_LEVELS_EXPORTS)
    assert all(hasattr(lib, name) for name in LEVELS)


def test_module_exports_none_of_them_and_its_list_is_the_main_headers():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert not set(capi.MAP_LEVELS_EXPORTS) & exported and lib.vgicp_abi_version() == 6
    assert "level" not in " ".join(sorted(exported))
    main = open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()
    assert "levels" not in main and "vgicp_hip_map_levels" not in main


def test_stats_layout_matches_the_header(tmp_path):
    assert C.sizeof(capi.LevelsStats) == 104
    assert [f for f, _ in capi.LevelsStats._fields_] == list(STATS_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_map_levels.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vgicp_levels_stats));\n' +
                   "".join(f'  printf(" %zu", offsetof(vgicp_levels_stats, {f}));\n' for f in STATS_FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [104] + [getattr(capi.LevelsStats, f).offset for f in STATS_FIELDS] == [104, 0, 40, 80, 84, 88, 96]


def test_entry_points_refuse_a_null_context_and_a_foreign_one_and_write_nothing():
    lib = capi.load_library()
    pose = (C.c_double * 16)(*np.eye(4).reshape(16))
    out = (C.c_double * 16)(*([7.0] * 16))
    params = capi.Params(10, 0, 1e-6, 0.9999, 0, 0)
    level = (C.c_int32 * 1)(0)
    stats = capi.LevelsStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    before = bytes(stats)
    v, s, h, w = C.c_size_t(7), C.c_size_t(7), C.c_double(7.0), C.c_size_t(7)
    foreign = C.create_string_buffer(4096)       # a block that no build of the module stamped
    for ctx in (None, C.cast(foreign, C.c_void_p)):
        assert lib.vgicp_map_levels_build(ctx, 2, C.byref(stats)) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_map_level_size(ctx, 0, C.byref(v), C.byref(s), C.byref(h)) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_map_level_export(ctx, 0, 0, None, None, None, None, C.byref(w)) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_align_resident_levels(ctx, pose, 1, level, C.byref(params), out, None) == capi.ERR_BAD_ARGUMENT
        if ctx is not None:
            assert "not from one build" in lib.vgicp_last_error(None).decode()
    assert bytes(stats) == before and (v.value, s.value, h.value, w.value) == (7, 7, 7.0, 7) and list(out) == [7.0] * 16
    assert foreign.raw == bytes(4096)


# ---- the host plan ----------------------------------------------------------------------------------------------------
def test_plan_levels_refuses_in_the_headers_order(tmp_path):
    """tests/native/levels_plan.cpp: the first rule that applies, over every combination of the facts and entries."""
    out = native(tmp_path, "levels_plan", os.path.join(ROOT, "eskf_lio_amd", "csrc")).strip()
    assert out.startswith("ok ") and "MISMATCH" not in out, out
    counts = [int(v) for v in re.findall(r"rule \d (\d+)", out)]
    assert len(counts) == 8 and all(c > 0 for c in counts), out          # every rule is reached
    assert int(re.search(r"passed (\d+)", out).group(1)) > 0
    header = open(os.path.join(ROOT, "include", "vgicp_hip_map_levels.h")).read()
    assert re.findall(r"^ \*   (\d)\. ", header, flags=re.M) == [str(k) for k in range(1, 9)]


# ---- the shim and the replay tool --------------------------------------------------------------------------------------
def test_shim_levels_over_a_stubbed_abi(tmp_path):
    """tests/native/shim_levels.cpp: LocalMap::setLevels and ICP::setCoarseToFine / alignCoarseToFine against a stand-in of
    the C ABI that records the calls — the stages' levels and thresholds, the per-stage report, the refusals, and no call
    of the new header while nothing is set (tests/golden/shim_routes.txt, held by tests/test_capi_cpu.py, is unchanged)."""
    exe = tmp_path / "shim_levels"
    cmd = ["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_levels.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout[-1000:] + run.stderr[-500:]
    lmap = open(os.path.join(ROOT, "include", "eskf_lio_shim", "LocalMap.hpp")).read()
    icp = open(os.path.join(ROOT, "include", "eskf_lio_shim", "Registration.hpp")).read()
    for name in ("void setLevels(int levels)", "#pragma weak vgicp_map_levels_build", '["coarse_to_fine"]["levels"]'):
        assert name in lmap, name
    for name in ("alignCoarseToFine(", "#pragma weak vgicp_align_resident_levels", 'reg["coarse_to_fine"]', 'ctf["coarse"]'):
        assert name in icp, name


def test_replay_flags_parse_and_only_the_device_backend_takes_them(oracle):
    import importlib.util
    from eskf_lio_amd import replay
    from replay_backends import OracleBackend
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert replay.coarse_to_fine_of(replay.DEFAULT_CONFIG) is None
    assert "coarse_to_fine" not in replay.DEFAULT_CONFIG["registration"]
    args = tool.parse_args(["--synthetic", "2", "--resident", "--levels", "3,2,1,0", "--coarse-max-iteration", "12",
                            "--coarse-translation-sq-threshold", "2e-4", "--coarse-cosine-threshold", "0.998"])
    cfg = tool.coarse_to_fine_config(replay.DEFAULT_CONFIG, args)
    assert replay.coarse_to_fine_of(cfg) == ([3, 2, 1, 0], dict(max_iteration=12, translation_sq_threshold=2e-4, cosine_threshold=0.998))
    only = tool.coarse_to_fine_config(replay.DEFAULT_CONFIG, tool.parse_args(["--synthetic", "2", "--resident", "--levels", "1,0"]))
    assert replay.coarse_to_fine_of(only) == ([1, 0], dict(max_iteration=30, translation_sq_threshold=1e-4, cosine_threshold=0.999))
    assert tool.coarse_to_fine_config(replay.DEFAULT_CONFIG, tool.parse_args(["--synthetic", "2", "--resident"])) is replay.DEFAULT_CONFIG
    reg = replay.DEFAULT_CONFIG["registration"]
    for bad in (dict(levels=[]), dict(levels=[5]), dict(levels=[-1, 0]), dict(levels=[0] * 9), dict(coarse={}),
                dict(levels=[1, 0], coarse=dict(max_iteration=-1)), dict(levels=[1, 0], coarse=dict(rounds=3)),
                dict(levels=[1, 0], stages=2)):
        with pytest.raises(ValueError, match="registration.coarse_to_fine"):
            replay.coarse_to_fine_of(dict(replay.DEFAULT_CONFIG, registration=dict(reg, coarse_to_fine=bad)))
    with pytest.raises(ValueError, match="coarse_to_fine"):
        replay.Odometry(cfg, OracleBackend(cfg, oracle))
    for argv in (["--synthetic", "2", "--levels", "1,0"], ["--synthetic", "2", "--resident", "--coarse-max-iteration", "5"]):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)


# ---- the rule: the restatement against brute-force properties ----------------------------------------------------------
def straddling_map(seed=5, n=400, span=6):
    """A map with keys on both sides of 0 in every axis, counts that differ between siblings, full covariances."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(-span, span, size=(n, 3)), axis=0).astype(np.int32)
    m = len(keys)
    means = (keys + rng.random((m, 3))) * ml.VOXEL
    a = rng.standard_normal((m, 3, 3)) * 0.05
    covs = (a @ a.transpose(0, 2, 1) + 1e-4 * np.eye(3)).reshape(m, 9)
    counts = rng.integers(1, 50, size=m).astype(np.uint64)
    return keys, means, covs, counts


def test_level_keys_are_the_unique_shifted_keys_and_counts_add_up():
    keys, means, covs, counts = straddling_map()
    assert (keys.min(axis=0) < 0).all() and (keys.max(axis=0) > 0).all()
    levels = ml.levels_of(keys, means, covs, counts, ml.LEVELS_MAX)
    for l, lv in enumerate(levels):
        want = np.unique(keys.astype(np.int64) >> l, axis=0)
        assert np.array_equal(lv.keys, want), l
        assert int(lv.counts.sum()) == int(counts.sum())
        # brute force, voxel by voxel: the count is the sum over the level-0 voxels that shift to the key
        for k, n in zip(lv.keys[:40], lv.counts[:40]):
            assert int(n) == int(counts[np.all((keys.astype(np.int64) >> l) == k, axis=1)].sum())
    assert len(levels[-1]) < len(levels[1]) < len(levels[0])
    assert np.array_equal(np.array([-1, -2, -3, 0, 1]) >> 1, [-1, -1, -2, 0, 0])          # arithmetic: -1 -> -1


def test_a_one_child_voxel_is_the_childs_bits_and_a_merge_is_the_weighted_mean():
    keys, means, covs, counts = straddling_map()
    fine = ml.as_level(keys, means, covs, counts)
    coarse = ml.coarsen(fine)
    parent = fine.keys.astype(np.int64) >> 1
    singles = merged = 0
    for i, k in enumerate(coarse.keys):
        kids = np.flatnonzero(np.all(parent == k, axis=1))
        octant = (fine.keys[kids] & 1) @ np.array([1, 2, 4])
        kids = kids[np.argsort(octant)]
        if len(kids) == 1:
            c = kids[0]
            assert coarse.means[i].tobytes() == fine.means[c].tobytes() and coarse.covs[i].tobytes() == fine.covs[c].tobytes()
            assert coarse.counts[i] == fine.counts[c]
            singles += 1
            continue
        merged += 1
        # the rule with Python floats, one operation at a time, in octant order
        n = sum(int(fine.counts[c]) for c in kids)
        for e in range(12):
            vals = [float(np.concatenate([fine.means[c], fine.covs[c]])[e]) for c in kids]
            acc = float(int(fine.counts[kids[0]])) * vals[0]
            for c, x in zip(kids[1:], vals[1:]):
                acc = acc + float(int(fine.counts[c])) * x
            got = coarse.means[i][e] if e < 3 else coarse.covs[i][e - 3]
            assert got == acc / float(n)
        # ... and up to rounding it is the exact weighted mean
        w = fine.counts[kids].astype(np.float64)
        assert np.allclose(coarse.means[i], (w[:, None] * fine.means[kids]).sum(axis=0) / w.sum(), rtol=1e-14, atol=0)
    assert singles > 20 and merged > 20


def test_symmetric_children_give_a_bitwise_symmetric_covariance():
    keys, means, covs, counts = straddling_map()
    c = covs.reshape(-1, 3, 3)
    assert all(np.array_equal(x, x.T) for x in c)          # a @ a.T + diag is bitwise symmetric
    for lv in ml.levels_of(keys, means, covs, counts, ml.LEVELS_MAX)[1:]:
        m = lv.covs.reshape(-1, 3, 3)
        assert m.tobytes() == m.transpose(0, 2, 1).copy().tobytes()


def test_all_eight_children_around_the_origin():
    """Keys -2 .. 1 on every axis fully occupied: the parents straddle 0 and have all eight children."""
    g = np.arange(-2, 2)
    keys = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    rng = np.random.default_rng(2)
    means = (keys + rng.random((64, 3))) * ml.VOXEL
    covs = np.tile(np.eye(3).reshape(9), (64, 1)) * rng.random((64, 1))
    counts = rng.integers(1, 9, size=64).astype(np.uint64)
    l0, l1, l2, l3 = ml.levels_of(keys, means, covs, counts, 3)
    assert len(l1) == 8 and sorted(map(tuple, l1.keys.tolist())) == [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
    assert len(l2) == 8 and len(l3) == 8          # -1 >> 1 == -1: the negative side never folds into 0
    assert int(l1.counts.sum()) == int(counts.sum()) and ml.same_level(l2, ml.Level(l1.keys, l1.means, l1.covs, l1.counts))


# ---- the key identity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel", (0.3, 0.05, 1.0, 0.7))
def test_a_levels_key_is_the_maps_key_shifted(oracle, voxel):
    """floor(fl(x / (h 2^l))) == floor(fl(x / h)) >> l: the quotient by h 2^l IS the quotient by h scaled by 2^-l, exactly,
    as long as it does not underflow, so the oracle's key function addresses a level without change — also a few ulps
    either side of a voxel face and for negative coordinates.  Around the face at 0 "a few ulps" are subnormal numbers:
    those are the next test's; here the face at 0 gets the smallest NORMAL numbers on either side."""
    rng = np.random.default_rng(7)
    faces = np.arange(-40, 41).astype(np.float64) * voxel
    near = [faces]
    for _ in range(4):
        f = near[-1]
        near.append(np.nextafter(f, np.inf))
    f = faces
    for _ in range(4):
        f = np.nextafter(f, -np.inf)
        near.append(f)
    near = np.concatenate(near + [np.arange(-40, 41) * (voxel * 16.0), np.nextafter(np.arange(-40, 41) * (voxel * 16.0), -np.inf)])
    tiny = np.finfo(np.float64).tiny * 64.0          # x / (h 16) stays a normal number
    near = near[(near == 0.0) | (np.abs(near) >= tiny)]
    x = np.concatenate([near, [tiny, -tiny, 2 * tiny, -2 * tiny, -0.0], rng.uniform(-60.0, 60.0, 4000)])
    pts = np.stack([x, x[::-1], np.roll(x, 17)], axis=1)
    k0 = oracle.voxel_index(voxel, pts).astype(np.int64)
    assert (k0 < 0).any() and (k0 > 0).any()
    for l in range(1, ml.LEVELS_MAX + 1):
        assert np.array_equal(oracle.voxel_index(voxel * 2 ** l, pts).astype(np.int64), k0 >> l), (voxel, l)


def test_the_identity_ends_where_the_quotient_underflows(oracle):
    """The one exception, written down so that nobody has to find it again: a NEGATIVE coordinate so close to 0 that its
    quotient by the level's voxel size underflows to -0 (|x| below 2^-1074 h 2^l, some 1e-323 m) has the map key -1 and
    the level key 0.  No sensor returns such a coordinate, and a point there matches a neighbouring voxel's record."""
    x = -np.finfo(np.float64).smallest_subnormal
    pts = np.array([[x, x, x]])
    assert oracle.voxel_index(0.3, pts).tolist() == [[-1, -1, -1]]
    assert oracle.voxel_index(0.3 * 8, pts).tolist() == [[0, 0, 0]]
    assert oracle.voxel_index(0.3 * 8, -pts).tolist() == oracle.voxel_index(0.3, -pts).tolist() == [[0, 0, 0]]


# ---- the oracle can align against a level, unchanged ------------------------------------------------------------------
@pytest.fixture(scope="module")
def experiment(oracle):
    """The recipe of the coarse-to-fine experiment: map, scan, levels 0 .. 3 as oracle maps, P*."""
    mp, mc, sp, sc = ml.recipe(oracle)
    omap = oracle.OracleMap(ml.VOXEL, ml.CAP)
    omap.insert(mp, mc)
    levels = ml.levels_of(*omap.export(), 3)
    maps = [omap] + [ml.oracle_level_map(oracle, levels[l], ml.VOXEL * 2 ** l) for l in (1, 2, 3)]
    star = omap.align(sp, sc, np.eye(4), ml.FINE["max_iteration"], ml.FINE["translation_sq_threshold"], ml.FINE["cosine_threshold"])
    return levels, maps, sp, sc, star.pose


def test_an_oracle_map_of_the_levels_size_holds_exactly_the_levels_keys(oracle, experiment):
    levels, maps, _, _, _ = experiment
    assert [len(lv) for lv in levels] == [15364, 10090, 5872, 2713]
    for l in (1, 2, 3):
        keys, means, covs, _ = maps[l].export()
        got = ml.as_level(keys, means, covs, np.ones(len(keys), dtype=np.uint64))
        assert np.array_equal(got.keys, levels[l].keys)
        assert got.means.tobytes() == levels[l].means.tobytes() and got.covs.tobytes() == levels[l].covs.tobytes()


# ---- the point of it --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", ml.SHIFTS)
def test_the_chain_converges_where_the_plain_align_sits_in_another_voxel(oracle, experiment, dx):
    """Measured here: the plain align ends 0.257, 0.624, 0.900, 1.222 m from P*, the chain 3 -> 2 -> 1 -> 0 1.1 - 1.2 mm
    (the fine stage's own stopping distance).  The limits are conditions stated in voxels, not tuned numbers."""
    _, maps, sp, sc, star = experiment
    guess = ml.shifted(dx)
    plain = maps[0].align(sp, sc, guess, ml.FINE["max_iteration"], ml.FINE["translation_sq_threshold"], ml.FINE["cosine_threshold"])
    pose, stages = ml.oracle_chain(oracle, maps, sp, sc, guess)
    far, near = ml.distance(plain.pose, star), ml.distance(pose, star)
    print(f"shift {dx} m: plain {far:.4f} m, chain {1e3 * near:.3f} mm from P*, rounds {[s.iterations for s in stages]}")
    assert far >= ml.FAR_LIMIT
    assert near <= ml.NEAR_LIMIT


def test_a_shorter_schedule_fails_earlier_and_level_3_reaches_no_further_than_its_width(oracle, experiment):
    _, maps, sp, sc, star = experiment
    pose, _ = ml.oracle_chain(oracle, maps, sp, sc, ml.shifted(0.3), schedule=(2, 1, 0))
    assert ml.distance(pose, star) >= ml.FAR_LIMIT
    pose, _ = ml.oracle_chain(oracle, maps, sp, sc, ml.shifted(1.8))
    assert ml.distance(pose, star) >= ml.FAR_LIMIT
