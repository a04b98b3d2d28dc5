"""The ray report (include/vgicp_hip_map_rays.h) without a device: the header against the Python mirror, the libraries'
exports, the host plan (plan_rays' refusals in their order, the groups), the shim against a stand-in of the C ABI, the
replay flags, and the reference of tests/test_map_rays.py checked on its own: against free-space carving's walk, against a
brute-force first hit, hand-made rays, and the room scene's classes on the committed seeds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_carve_reference as mc
import map_rays_reference as mr
from eskf_lio_amd import capi
from test_evaluate_cpu import declared
from test_map_gated_cpu import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS_FIELDS = ("origin", "margin", "beyond", "max_range", "stride", "reserved")
OUTPUT_FIELDS = ("status", "range", "hit_key", "steps")
COUNTS_FIELDS = ("rays", "visits", "by_class")
STATS_FIELDS = ("launches", "groups", "seconds", "device_seconds")


# ---- header and libraries ---------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_function_and_the_library_exports_it():
    lib = capi.load_library()
    assert declared("vgicp_hip_map_rays.h") == sorted(capi.MAP_RAYS_EXPORTS) == ["vgicp_rays_resident"]
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_rays.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_map_rays.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    assert re.search(r"#define\s+VGICP_RAYS_MAX_POSES\s+%d\b" % capi.RAYS_MAX_POSES, text)
    for value, name in enumerate(("NO_RAY", "OPEN", "OWN", "BEHIND", "CONFIRMED", "BLOCKED", "NEAR")):
        assert re.search(r"VGICP_RAY_%s = %d\b" % (name, value), text) and getattr(capi, "RAY_" + name) == getattr(mr, name) == value
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("map_rays")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.MAP_RAYS_EXPORTS)
    assert hasattr(lib, "vgicp_rays_resident")


def test_module_exports_stay_as_they_are():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert not set(capi.MAP_RAYS_EXPORTS) & exported and lib.vgicp_abi_version() == 6
    assert "vgicp_rays" not in open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()


def test_layouts_match_the_header(tmp_path):
    sizes = [C.sizeof(capi.RayParams), C.sizeof(capi.RayOutputs), C.sizeof(capi.RayCounts), C.sizeof(capi.RayStats)]
    assert sizes == [56, 32, 80, 24]
    structs = (("vgicp_ray_params", capi.RayParams, PARAMS_FIELDS), ("vgicp_ray_outputs", capi.RayOutputs, OUTPUT_FIELDS),
               ("vgicp_ray_counts", capi.RayCounts, COUNTS_FIELDS), ("vgicp_ray_stats", capi.RayStats, STATS_FIELDS))
    for _, cls, fields in structs:
        assert [f for f, _ in cls._fields_] == list(fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_map_rays.h"\nint main(void) {\n' +
                   "".join(f'  printf(" %zu", sizeof({name}));\n' for name, _, _ in structs) +
                   "".join(f'  printf(" %zu", offsetof({name}, {f}));\n' for name, _, fields in structs for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == sizes + [getattr(cls, f).offset for _, cls, fields in structs for f in fields]
    assert got[4:] == [0, 24, 32, 40, 48, 52] + [0, 8, 16, 24] + [0, 8, 16] + [0, 4, 8, 16]


def test_entry_point_refuses_a_null_context_and_a_foreign_one_and_writes_nothing():
    lib = capi.load_library()
    pose = (C.c_double * 16)(*np.eye(4).reshape(16))
    params = capi.ray_params()
    stats, counts = capi.RayStats(), capi.RayCounts()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    C.memset(C.byref(counts), 0xA5, C.sizeof(counts))
    before = bytes(stats), bytes(counts)
    status = (C.c_uint8 * 4)(*([0x5A] * 4))
    out = capi.RayOutputs(status, None, None, None)
    foreign = C.create_string_buffer(4096)       # a block that no build of the module stamped
    for ctx in (None, C.cast(foreign, C.c_void_p)):
        assert lib.vgicp_rays_resident(ctx, pose, 1, C.byref(params), C.byref(out), C.byref(counts), C.byref(stats)) == capi.ERR_BAD_ARGUMENT
        if ctx is not None:
            assert "not from one build" in lib.vgicp_last_error(None).decode()
    assert (bytes(stats), bytes(counts)) == before and list(status) == [0x5A] * 4 and foreign.raw == bytes(4096)


# ---- the host plan and the shim -----------------------------------------------------------------------------------------
def test_plan_rays_refuses_in_the_headers_order(tmp_path):
    """tests/native/map_rays_plan.cpp: the first rule that applies, over every combination of the facts; the groups."""
    out = native(tmp_path, "map_rays_plan", os.path.join(ROOT, "eskf_lio_amd", "csrc")).strip()
    assert out.startswith("ok 1179661 checks:") and out.endswith("passed 576"), out
    # every rule is reached
    reached = re.findall(r"rule (\d+) (\d+)", out)
    assert [int(r) for r, _ in reached] == list(range(3, 12)) and all(int(v) > 0 for _, v in reached)
    header = open(os.path.join(ROOT, "include", "vgicp_hip_map_rays.h")).read()
    rules = re.findall(r"^ \* +(\d+)\. ", header, flags=re.M)
    assert rules == [str(k) for k in range(1, 12)]
    # carving's plan is what it was
    assert native(tmp_path, "map_carve_plan", os.path.join(ROOT, "eskf_lio_amd", "csrc")).startswith("ok 17284 verdicts:")


def test_shim_ray_report_against_a_stand_in(tmp_path):
    """tests/native/shim_rays.cpp: LocalMap::rayReport / rayCounts against a stubbed C ABI.  With no resident scan (and on
    a host-authoritative map) the result says available == false and nothing throws."""
    exe = tmp_path / "shim_rays"
    cmd = ["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_rays.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout[-1000:] + run.stderr[-500:]
    shim = open(os.path.join(ROOT, "include", "eskf_lio_shim", "LocalMap.hpp")).read()
    for name in ("rayReport(", "rayCounts(", "#pragma weak vgicp_rays_resident", "available"):
        assert name in shim, name


def test_replay_flags_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args(["--synthetic", "2", "--resident", "--ray-report", "40", "--ray-margin", "0.5", "--ray-beyond", "10",
                            "--ray-stride", "4"])
    assert tool.ray_report_params(args) == dict(max_range=40.0, margin=0.5, beyond=10.0, stride=4)
    assert tool.ray_report_params(tool.parse_args(["--synthetic", "2", "--resident", "--ray-report", "30"])) == \
        dict(max_range=30.0, margin=0.0, beyond=0.0, stride=1)
    assert tool.ray_report_params(tool.parse_args(["--synthetic", "2", "--resident"])) is None
    for bad in (["--ray-report", "40"], ["--resident", "--ray-margin", "1"]):          # needs --resident; needs --ray-report
        with pytest.raises(SystemExit):
            tool.parse_args(["--synthetic", "2"] + bad)


# ---- the reference on its own: hand-made rays -------------------------------------------------------------------------
H = 0.5
EYE = np.eye(4)
START = (0.25, 0.25, 0.25)            # the centre of voxel (0, 0, 0)
NAN_BITS = np.uint64(mr.NO_HIT_RANGE_BITS)


def row(*xs):
    return np.array([[x, 0, 0] for x in xs], dtype=np.int64)


def test_the_walk_stops_at_the_first_full_voxel_and_classes_follow_the_order():
    keys = row(4, 6)                                   # voxels [2.0, 2.5) and [3.0, 3.5) on the x axis
    p = mr.Params(margin=0.4, beyond=5.0, origin=START)
    pts = [[2.25, 0.25, 0.25],      # in voxel 4: OWN
           [1.25, 0.25, 0.25],      # in front of it: the hit lies behind the return: BEHIND
           [2.75, 0.25, 0.25],      # behind voxel 4, hit 0.75 in front of the return, voxel 4 holds point 0: CONFIRMED
           [9.25, 0.25, 0.25]]      # far behind: still voxel 4 (the first FULL one), confirmed
    r = mr.rays(keys, H, pts, EYE, p)
    assert r.status.tolist() == [mr.OWN, mr.BEHIND, mr.CONFIRMED, mr.CONFIRMED]
    assert r.hit_key.tolist() == [[4, 0, 0]] * 4 and r.steps.tolist() == [5, 5, 5, 5] and r.range.tolist() == [1.75] * 4
    # without point 0 nothing confirms voxel 4: BLOCKED in front of the margin, NEAR within it
    r = mr.rays(keys, H, pts[1:], EYE, p)
    assert r.status.tolist() == [mr.BEHIND, mr.BLOCKED, mr.BLOCKED]
    r = mr.rays(keys, H, pts[1:], EYE, mr.Params(margin=0.8, beyond=5.0, origin=START))
    assert r.status.tolist() == [mr.BEHIND, mr.NEAR, mr.BLOCKED]
    # beyond = 0: the ray of point 1 ends at its return: OPEN, NaN, INT32_MIN, 3 voxels visited
    r = mr.rays(keys, H, pts[1:2], EYE, mr.Params(origin=START))
    assert r.status.tolist() == [mr.OPEN] and r.range.view(np.uint64).tolist() == [NAN_BITS] and r.steps.tolist() == [3]
    assert r.hit_key.tolist() == [[mr.NO_HIT_KEY] * 3] and r.counts() == dict(rays=1, visits=3, by_class=[0, 1, 0, 0, 0, 0, 0, 0])
    # max_range shorter than the return: the ray ends inside voxel 2, in front of everything
    r = mr.rays(keys, H, pts[:1], EYE, mr.Params(beyond=5.0, max_range=1.0, origin=START))
    assert r.status.tolist() == [mr.OPEN] and r.steps.tolist() == [3]


def test_corners_of_the_rule_on_the_reference():
    # a FULL voxel at key(o): t_in = 0, range 0, one voxel visited; OWN only for the return inside it
    r = mr.rays(row(0), H, [[2.25, 0.25, 0.25], [0.4, 0.3, 0.25]], EYE, mr.Params(origin=START))
    assert r.status.tolist() == [mr.CONFIRMED, mr.OWN] and r.range.tolist() == [0.0, 0.0] and r.steps.tolist() == [1, 1]
    r = mr.rays(row(0), H, [[2.25, 0.25, 0.25]], EYE, mr.Params(origin=START))
    assert r.status.tolist() == [mr.BLOCKED] and r.range.tolist() == [0.0]
    # a point at the origin (len = 0), NaN and infinite coordinates: no ray, no confirmation
    bad = [[1.25, 0.25, 0.25], [np.nan, 0.25, 0.25], [np.inf, 0.25, 0.25], [2.25, 0.25, 0.25]]
    r = mr.rays(row(0, 4), H, bad, EYE, mr.Params(origin=(1.25, 0.25, 0.25)))
    assert r.status.tolist() == [mr.NO_RAY] * 3 + [mr.OWN] and r.steps.tolist() == [0, 0, 0, 3]
    assert r.counts()["by_class"][:3] == [3, 0, 1]
    # ... but the point at the origin still confirms its voxel for the others
    r = mr.rays(row(0), H, [list(START), [2.25, 0.25, 0.25]], EYE, mr.Params(origin=START))
    assert r.status.tolist() == [mr.NO_RAY, mr.CONFIRMED] and r.steps.tolist() == [0, 1]
    # a ray along -x: the return's voxel is OWN, a return behind it finds it confirmed
    r = mr.rays(row(0), H, [list(START), [-1.25, 0.25, 0.25]], EYE, mr.Params(origin=(1.25, 0.25, 0.25)))
    assert r.status.tolist() == [mr.OWN, mr.CONFIRMED] and r.steps.tolist() == [3, 3] and r.range.tolist() == [0.75, 0.75]
    # the diagonal from a voxel corner region: x, then y, then z
    keys = np.array([[1, 1, 1]], dtype=np.int64)
    r = mr.rays(keys, H, [[0.75, 0.75, 0.75]], EYE, mr.Params(origin=START))
    assert r.status.tolist() == [mr.OWN] and r.steps.tolist() == [4] and r.range.tolist() == [0.5 * np.sqrt(0.75)]
    # key(o) out of range: no ray at all; an empty map: every ray OPEN
    far = np.eye(4)
    far[0, 3] = 2.0 ** 30
    r = mr.rays(row(0), H, [[2.25, 0.25, 0.25]], far, mr.Params(origin=START))
    assert r.status.tolist() == [mr.NO_RAY]
    r = mr.rays(np.zeros((0, 3), dtype=np.int64), H, [[2.25, 0.25, 0.25], [0.3, 1.0, -2.0]], EYE, mr.Params(origin=START, beyond=3.0))
    assert r.status.tolist() == [mr.OPEN, mr.OPEN] and r.steps.min() > 5


def test_stride_picks_the_rays_and_every_point_confirms():
    keys = row(4)
    pts = [[3.25, 0.25, 0.25], [2.25, 0.25, 0.25], [2.3, 0.3, 0.25], [3.75, 0.3, 0.3]]
    r = mr.rays(keys, H, pts, EYE, mr.Params(origin=START, stride=3))
    assert r.status.tolist() == [mr.CONFIRMED, mr.NO_RAY, mr.NO_RAY, mr.CONFIRMED] and r.counts()["rays"] == 2
    assert r.counts()["by_class"] == [2, 0, 0, 0, 2, 0, 0, 0]


# ---- the reference on its own: the scene ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return {seed: mr.make_scene(max(mr.SIZES), seed) for seed in mr.SCENE_SEEDS}


def test_the_room_is_what_the_scene_says(scenes):
    room = scenes[mr.SCENE_SEEDS[0]][0]
    shell = (2 * mr.SHELL + 1) ** 3 - (2 * mr.SHELL - 1) ** 3 - (2 * mr.WINDOW + 1) ** 2
    assert len(room.keys) == shell + mr.STALE and len(np.unique(room.keys, axis=0)) == len(room.keys) and shell == 13745
    o = mr.transform(mr.scene_pose(), np.asarray(mr.ORIGIN))[0]
    away = np.sqrt((((room.stale + 0.5) * mr.VOXEL - o) ** 2).sum(axis=1))
    assert 2.5 < away.min() and away.max() < 8.5


@pytest.mark.parametrize("seed", mr.SCENE_SEEDS)
def test_visits_at_beyond_zero_are_carvings_cut_after_the_first_full_voxel(scenes, seed):
    """One definition of the step: at beyond = 0 the report's ray is carving's at margin = 0, up to the first FULL voxel."""
    room, pts, T = scenes[seed]
    pts = pts[:1000]
    r = mr.rays(room.keys, mr.VOXEL, pts, T, mr.Params(origin=mr.ORIGIN))
    ray, key, steps, _ = mc.walk(pts, T, mr.VOXEL, mc.Params(origin=mr.ORIGIN))
    full = mc.match(room.keys, key) >= 0
    cut, total = 0, 0
    mine_ray, mine_key = r.visit_ray, r.visit_key
    for i in range(len(pts)):
        theirs = key[ray == i]                                   # in step order (walk appends step by step)
        hits = np.flatnonzero(full[ray == i])
        if len(hits):
            theirs = theirs[:hits[0] + 1]
            cut += 1
        mine = mine_key[mine_ray == i]
        assert mine.shape == theirs.shape and np.array_equal(mine, theirs), i
        assert r.steps[i] == len(theirs) and (r.hit[i] >= 0) == bool(len(hits))
        total += len(theirs)
    assert cut > 500 and total == r.counts()["visits"] and steps.sum() > total


@pytest.mark.parametrize("seed", mr.SCENE_SEEDS)
def test_brute_force_first_hit_agrees_on_every_ray_it_can_decide(scenes, seed):
    """The slab method over every (ray, voxel) pair: nothing of the traversal's step order in it.  At most 1 % of the rays
    may be undecidable on the committed seeds (a ray within 2e-7 voxel sizes of an edge); the scene stays at 0."""
    room, pts, T = scenes[seed]
    pts = pts[:1000 if seed == mr.SCENE_SEEDS[0] else 300]
    p = mr.Params(margin=1.0, beyond=20.0, origin=mr.ORIGIN)
    r = mr.rays(room.keys, mr.VOXEL, pts, T, p)
    first, decided, casts = mr.first_hit_brute(room.keys, mr.VOXEL, pts, T, p)
    undecided = int(np.count_nonzero(casts & ~decided))
    print(f"seed {seed}: {int(casts.sum())} rays, {undecided} undecided, {r.counts()}")
    assert casts.sum() == len(pts) and undecided <= 0.01 * casts.sum()
    assert np.array_equal(first[casts & decided], r.hit[casts & decided])
    assert np.count_nonzero(first >= 0) > 0.8 * len(pts) and np.count_nonzero(first < 0) > 0.05 * len(pts)
    # the check can fail: a map without a ray's hit voxel gives that ray another first hit
    i = int(np.flatnonzero(r.hit >= 0)[0])
    less = np.delete(room.keys, r.hit[i], axis=0)
    again, _, _ = mr.first_hit_brute(less, mr.VOXEL, pts[i:i + 1], T, p)
    assert again[0] < 0 or not np.array_equal(less[again[0]], room.keys[r.hit[i]])


@pytest.mark.parametrize("seed", mr.SCENE_SEEDS)
def test_every_class_is_populated(scenes, seed):
    room, pts, T = scenes[seed]
    small = mr.rays(room.keys, mr.VOXEL, pts[:63], T, mr.Params(1.0, 20.0, mr.MAX_RANGE, 3, mr.ORIGIN)).counts()
    assert small["rays"] == 21 and all(c >= 1 for c in small["by_class"][1:7]), small
    large = mr.rays(room.keys, mr.VOXEL, pts, T, mr.Params(1.0, 20.0, mr.MAX_RANGE, 1, mr.ORIGIN))
    counts = large.counts()
    print(f"seed {seed}: n 63 stride 3 {small['by_class']}; n 3000 {counts['by_class']}; longest walk {large.steps.max()}")
    assert counts["rays"] == 3000 and all(c >= 0.02 * counts["rays"] for c in counts["by_class"][1:7]), counts
    assert counts["by_class"][0] == counts["by_class"][7] == 0 and large.steps.max() > 100
    # a prefix of a scan is a scan: the 63-point scan's kinds are all there
    assert sorted(set((np.arange(63) % 8).tolist())) == list(range(8))
