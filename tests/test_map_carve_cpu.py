"""Free-space carving (include/vgicp_hip_map_carve.h) without a device: the header against the Python mirror, the
libraries' exports, the host plans (plan_carve's refusals in their order, the shim's update plan with the new fact), the
replay flags, and the reference of tests/test_map_carve.py checked on its own: hand-made rays, and the brute-force
sandwich on the committed seeds, where it must also be tight."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_carve_reference as mc
from eskf_lio_amd import capi
from test_evaluate_cpu import declared
from test_map_gated_cpu import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARVE = ["vgicp_map_carve_resident", "vgicp_map_carve_resident_async", "vgicp_map_carve_totals"]
PARAMS_FIELDS = ("origin", "margin", "max_range", "min_hits", "stride")
STATS_FIELDS = ("rays", "visits", "touched", "shielded", "removed", "launches", "reserved", "seconds", "device_seconds")


# ---- header and libraries ---------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_three_functions_and_the_library_exports_them():
    lib = capi.load_library()
    assert declared("vgicp_hip_map_carve.h") == sorted(capi.MAP_CARVE_EXPORTS) == CARVE
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_carve.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_map_carve.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    assert re.search(r"#define\s+VGICP_CARVE_MAX_STEPS\s+%d\b" % capi.CARVE_MAX_STEPS, text) and mc.MAX_STEPS == capi.CARVE_MAX_STEPS
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("map_carve")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.MAP_CARVE_EXPORTS)
    assert all(hasattr(lib, name) for name in CARVE)


def test_module_exports_none_of_them():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert not set(capi.MAP_CARVE_EXPORTS) & exported and lib.vgicp_abi_version() == 6
    assert "carve" not in open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()


def test_layouts_match_the_header(tmp_path):
    assert C.sizeof(capi.CarveParams) == 48 and C.sizeof(capi.CarveStats) == 64
    assert [f for f, _ in capi.CarveParams._fields_] == list(PARAMS_FIELDS)
    assert [f for f, _ in capi.CarveStats._fields_] == list(STATS_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_map_carve.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(vgicp_carve_params), sizeof(vgicp_carve_stats));\n' +
                   "".join(f'  printf(" %zu", offsetof(vgicp_carve_params, {f}));\n' for f in PARAMS_FIELDS) +
                   "".join(f'  printf(" %zu", offsetof(vgicp_carve_stats, {f}));\n' for f in STATS_FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [48, 64] + [getattr(capi.CarveParams, f).offset for f in PARAMS_FIELDS] + \
        [getattr(capi.CarveStats, f).offset for f in STATS_FIELDS]
    assert got[2:] == [0, 24, 32, 40, 44] + [0, 8, 16, 24, 32, 40, 44, 48, 56]


def test_entry_points_refuse_a_null_context_and_a_foreign_one_and_write_nothing():
    lib = capi.load_library()
    pose = (C.c_double * 16)(*np.eye(4).reshape(16))
    params = capi.carve_params()
    stats = capi.CarveStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    before = bytes(stats)
    keys = (C.c_int32 * 6)(*([0x5A5A5A5A] * 6))
    removed, rays, gone = C.c_size_t(7), C.c_uint64(7), C.c_uint64(7)
    foreign = C.create_string_buffer(4096)       # a block that no build of the module stamped
    for ctx in (None, C.cast(foreign, C.c_void_p)):
        assert lib.vgicp_map_carve_resident(ctx, pose, C.byref(params), 2, keys, C.byref(removed), C.byref(stats)) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_map_carve_resident_async(ctx, pose, C.byref(params)) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_map_carve_totals(ctx, C.byref(rays), C.byref(gone)) == capi.ERR_BAD_ARGUMENT
        if ctx is not None:
            assert "not from one build" in lib.vgicp_last_error(None).decode()
    assert bytes(stats) == before and list(keys) == [0x5A5A5A5A] * 6 and (removed.value, rays.value, gone.value) == (7, 7, 7)
    assert foreign.raw == bytes(4096)


# ---- the host plans ---------------------------------------------------------------------------------------------------
def test_plan_carve_refuses_in_the_headers_order(tmp_path):
    """tests/native/map_carve_plan.cpp: the first rule that applies, over every combination of the facts."""
    out = native(tmp_path, "map_carve_plan", os.path.join(ROOT, "eskf_lio_amd", "csrc")).strip()
    assert out.startswith("ok 17284 verdicts:") and out.endswith("passed 36"), out
    # every rule is reached
    assert all(int(v) > 0 for v in re.findall(r"rule \d (\d+)", out)) and len(re.findall(r"rule \d", out)) == 7
    header = open(os.path.join(ROOT, "include", "vgicp_hip_map_carve.h")).read()
    rules = re.findall(r"^ \*   (\d)\. ", header, flags=re.M)
    assert rules == [str(k) for k in range(1, 10)]


def test_shim_plan_with_carve(tmp_path):
    """tests/native/update_plan_carve.cpp: carve = false reproduces today's plan for every combination of the old facts;
    carve = true adds plan.carve on the resident route with an insertion due and nowhere else."""
    out = native(tmp_path, "update_plan_carve", os.path.join(ROOT, "include"))
    assert out.strip() == "ok 2240 plans, 1216 identical without carve, 448 carve before the insertion"
    assert native(tmp_path, "update_plan", os.path.join(ROOT, "include")).startswith("ok ")
    assert native(tmp_path, "update_plan_gated", os.path.join(ROOT, "include")).startswith("ok ")
    shim = open(os.path.join(ROOT, "include", "eskf_lio_shim", "LocalMap.hpp")).read()
    for name in ("setCarve", "clearCarve", "carveTotals()", 'm["carve"]', "vgicp_map_carve_resident_async", "plan.carve"):
        assert name in shim, name


def test_replay_flags_parse_and_the_oracle_backend_refuses_them(oracle):
    import importlib.util
    from eskf_lio_amd import replay
    from replay_backends import OracleBackend
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert replay.carve_of(replay.DEFAULT_CONFIG) is None
    args = tool.parse_args(["--synthetic", "2", "--resident", "--carve-range", "40", "--carve-margin", "0.5", "--carve-min-hits", "2",
                            "--carve-stride", "4"])
    cfg = tool.carve_config(replay.DEFAULT_CONFIG, args)
    assert replay.carve_of(cfg) == dict(margin=0.5, max_range=40.0, min_hits=2, stride=4, origin=None)
    assert tool.carve_config(replay.DEFAULT_CONFIG, tool.parse_args(["--synthetic", "2", "--resident"])) is replay.DEFAULT_CONFIG
    for bad in (dict(max_range=0.0), dict(max_range=40.0, margin=-1.0), dict(max_range=40.0, min_hits=0),
                dict(max_range=40.0, stride=0)):
        with pytest.raises(ValueError, match="local_map.carve"):
            replay.carve_of(dict(replay.DEFAULT_CONFIG, local_map=dict(replay.DEFAULT_CONFIG["local_map"], carve=bad)))
    with pytest.raises(ValueError, match="carve"):
        replay.Odometry(cfg, OracleBackend(cfg, oracle))


# ---- the reference on its own: hand-made rays -------------------------------------------------------------------------
H = 0.5
EYE = np.eye(4)
START = (0.25, 0.25, 0.25)            # the centre of voxel (0, 0, 0)


def grid(nx, ny=1, nz=1):
    return np.array([[x, y, z] for x in range(nx) for y in range(ny) for z in range(nz)], dtype=np.int64)


def visited(keys, res):
    return sorted(map(tuple, keys[res.hits > 0].tolist()))


def test_axis_aligned_ray_through_a_row_of_five_voxels():
    keys = grid(8)
    res = mc.carve(keys, H, [[2.25, 0.25, 0.25]], EYE, mc.Params(origin=START))
    assert res.hits.tolist() == [1, 1, 1, 1, 1, 0, 0, 0] and res.counts() == dict(rays=1, visits=5, touched=5, shielded=1, removed=4)
    assert res.shield.tolist() == [False] * 4 + [True] + [False] * 3          # the return's own voxel stays
    assert res.removed.tolist() == [True] * 4 + [False] * 4
    # the same ray backwards (d < 0: the next boundary is the voxel's lower face)
    back = mc.carve(keys, H, [[0.25, 0.25, 0.25]], EYE, mc.Params(origin=(2.25, 0.25, 0.25)))
    assert back.hits.tolist() == res.hits.tolist() and back.removed.tolist() == [False] + [True] * 4 + [False] * 3


def test_direction_with_zero_components():
    """dy = dz = 0 above; here dz = 0 alone, and a ray along -z: an axis with d == 0 never steps (tMax = +inf)."""
    keys = grid(4, 4, 2)
    res = mc.carve(keys, H, [[1.75, 0.8, 0.25]], EYE, mc.Params(origin=START))
    seen = visited(keys, res)
    assert all(k[2] == 0 for k in seen) and seen[0] == (0, 0, 0) and seen[-1] == (3, 1, 0) and res.visits == len(seen) == 5
    down = mc.carve(grid(2, 2, 6) - [0, 0, 3], H, [[0.25, 0.25, -1.3]], EYE, mc.Params(origin=START))
    assert visited(grid(2, 2, 6) - [0, 0, 3], down) == [(0, 0, -3), (0, 0, -2), (0, 0, -1), (0, 0, 0)]


def test_ray_shorter_than_the_margin_is_no_ray_but_still_shields():
    keys = grid(8)
    for margin in (2.0, 2.5, 100.0):          # len == 2: min(len - margin, .) <= 0
        res = mc.carve(keys, H, [[2.25, 0.25, 0.25]], EYE, mc.Params(origin=START, margin=margin))
        assert res.counts() == dict(rays=0, visits=0, touched=0, shielded=0, removed=0) and res.shield[4]
    res = mc.carve(keys, H, [[2.25, 0.25, 0.25]], EYE, mc.Params(origin=START, margin=1.9))
    assert res.rays == 1 and res.visits == 1          # t_stop = 0.05: the ray never leaves the origin's voxel
    # a point at the origin itself: len == 0
    assert mc.carve(keys, H, [START], EYE, mc.Params(origin=START)).rays == 0


def test_max_range_cuts_a_ray_inside_a_voxel():
    keys = grid(8)
    res = mc.carve(keys, H, [[2.25, 0.25, 0.25]], EYE, mc.Params(origin=START, max_range=1.0))
    # the segment ends at x = 1.25, inside voxel 2 (entered at x = 1.0); voxel 3 would be entered at x = 1.5
    assert res.hits.tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and res.removed.tolist() == [True] * 3 + [False] * 5
    # ... exactly ON the boundary: entering at t == t_stop is not "< t_stop"
    res = mc.carve(keys, H, [[2.25, 0.25, 0.25]], EYE, mc.Params(origin=START, max_range=1.25))
    assert res.hits.tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    # the margin likewise: one voxel short of the return
    res = mc.carve(keys, H, [[2.25, 0.25, 0.25]], EYE, mc.Params(origin=START, margin=H))
    assert res.hits.tolist() == [1, 1, 1, 1, 0, 0, 0, 0] and res.shield[4] and not res.removed[4]


def test_tie_at_a_voxel_corner_takes_x_first():
    keys = grid(4, 4)
    res = mc.carve(keys, H, [[1.25, 1.25, 0.25]], EYE, mc.Params(origin=START))
    assert visited(keys, res) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0)]     # never (0, 1, 0) or (1, 2, 0)
    # all three at once: x, then y, then z
    keys = grid(3, 3, 3)
    res = mc.carve(keys, H, [[0.75, 0.75, 0.75]], EYE, mc.Params(origin=START))
    assert visited(keys, res) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]


def test_hits_count_distinct_rays_and_stride_picks_the_rays():
    keys = grid(8)
    pts = np.array([[2.25, 0.25, 0.25], [2.25, 0.3, 0.25], [1.3, 0.25, 0.3], [3.25, 0.25, 0.25]])
    res = mc.carve(keys, H, pts, EYE, mc.Params(origin=START, min_hits=3))
    assert res.hits.tolist() == [4, 4, 4, 3, 3, 1, 1, 0] and res.shield.tolist() == [False, False, True, False, True, False, True, False]
    assert res.removed.tolist() == [True, True, False, True, False, False, False, False]
    third = mc.carve(keys, H, pts, EYE, mc.Params(origin=START, stride=3))          # points 0 and 3 cast; all four shield
    assert third.rays == 2 and third.hits.tolist() == [2, 2, 2, 2, 2, 1, 1, 0] and third.shield.tolist() == res.shield.tolist()
    # a point that is not finite casts nothing and shields nothing
    bad = mc.carve(keys, H, [[np.nan, 0.25, 0.25], [np.inf, 0.25, 0.25]], EYE, mc.Params(origin=START))
    assert bad.counts() == dict(rays=0, visits=0, touched=0, shielded=0, removed=0) and not bad.shield.any()


# ---- the reference on its own: the sandwich -------------------------------------------------------------------------
SANDWICH_N = 400


@pytest.fixture(scope="module")
def vmap():
    from eskf_lio_amd import synth
    return synth.make_map(mc.MAP_VOXELS, voxel_size=mc.VOXEL)


@pytest.mark.parametrize("margin", mc.MARGINS)
@pytest.mark.parametrize("seed", mc.SCENE_SEEDS)
def test_reference_lies_inside_the_sandwich_and_the_sandwich_is_tight(vmap, seed, margin):
    """Brute force over every (ray, voxel) pair with a slab test: nothing of the traversal's step order in it.  On the
    committed seeds the voxels whose certain and possible counts differ are at most 0.1 % of the touched ones (zero is
    expected: a difference needs a ray within 1e-7 voxel sizes of a voxel's corner or edge)."""
    _, pts, T = mc.make_scene(SANDWICH_N, seed, vmap)
    assert np.abs(mc.transform(T, pts)).max() < 200.0
    p = mc.Params(margin=margin, origin=mc.ORIGIN)
    certain, possible = mc.slab_counts(vmap.keys, mc.VOXEL, pts, T, p)
    res = mc.carve(vmap.keys, mc.VOXEL, pts, T, p)
    loose = int(np.count_nonzero(certain != possible))
    print(f"seed {seed} margin {margin}: {res.counts()} undecided voxels {loose}")
    assert res.touched > 2000 and loose <= 0.001 * res.touched
    assert np.all(certain <= res.hits) and np.all(res.hits <= possible)
    for min_hits in mc.MIN_HITS:
        removed = (res.hits >= min_hits) & ~res.shield
        missed, wrong = mc.check_sandwich(removed, res.shield, certain, possible, min_hits)
        assert len(missed) == 0 and len(wrong) == 0 and removed.any()
    # the check can fail: a voxel taken out of / put into the removed set is found
    removed = res.removed.copy()
    flip = int(np.flatnonzero(removed)[0])
    removed[flip] = False
    assert mc.check_sandwich(removed, res.shield, certain, possible, 1)[0].tolist() == [flip]
    keep = int(np.flatnonzero(res.hits == 0)[0])
    removed = res.removed.copy()
    removed[keep] = True
    assert mc.check_sandwich(removed, res.shield, certain, possible, 1)[1].tolist() == [keep]


def test_a_ray_visits_a_voxel_at_most_once_and_within_the_step_bound(vmap):
    _, pts, T = mc.make_scene(1_000, mc.SCENE_SEEDS[0], vmap)
    p = mc.Params(origin=mc.ORIGIN)
    ray, key, steps, _ = mc.walk(pts, T, mc.VOXEL, p)
    rows = np.concatenate([ray[:, None], key], axis=1)
    assert len(np.unique(rows, axis=0)) == len(rows) == steps.sum()
    _, _, _, length, t_stop, casts = mc.rays_of(pts, T, p)
    bound = 3 * np.ceil(t_stop * length / mc.VOXEL) + 3
    assert np.all(steps[casts] - 1 < bound[casts]) and steps.max() > 100          # no ray is cut short by the bound
    # consecutive visits are face neighbours
    order = np.lexsort((np.arange(len(ray)), ray))
    same = ray[order][1:] == ray[order][:-1]
    assert np.all(np.abs(np.diff(key[order], axis=0)).sum(axis=1)[same] == 1)
