"""The gated map insertion (include/vgicp_hip_map_gated.h) without a device: the header against the Python mirror, the
libraries' exports, the host plans (the insertion entries' refusals, the gate's own rules, the shim's update plan with a
gate), the replay flag, and the preconditions of tests/test_map_gated.py, checked on the reference alone."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import map_gated_reference as mg
import points_reference as pr
import robust_reference as rr
from eskf_lio_amd import capi
from test_evaluate_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_FIELDS = ("points", "matched", "refused", "not_finite", "new_voxels", "launches", "reserved", "seconds",
                "device_seconds")
GATED = ["vgicp_map_gated_totals", "vgicp_map_insert_resident_gated", "vgicp_map_insert_resident_gated_async"]


# ---- header and libraries ---------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_three_functions_and_the_library_exports_them():
    lib = capi.load_library()
    assert declared("vgicp_hip_map_gated.h") == sorted(capi.MAP_GATED_EXPORTS) == GATED
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_gated.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_map_gated.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("map_gated")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.MAP_GATED_EXPORTS)
    assert all(hasattr(lib, name) for name in GATED)


def test_module_still_exports_exactly_the_four_pinned_lists():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    pinned = set(capi.EXPORTS) | set(capi.MAP_POINTS_EXPORTS) | set(capi.BATCH_EXPORTS) | set(capi.EVALUATE_EXPORTS)
    assert len(pinned) == 47 + 2 + 2 + 1 and exported == pinned
    assert not set(capi.MAP_GATED_EXPORTS) & pinned and lib.vgicp_abi_version() == 6
    main = open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()
    assert "gated" not in main


def test_layout_matches_the_header(tmp_path):
    assert C.sizeof(capi.GatedInsertStats) == 64
    assert [f for f, _ in capi.GatedInsertStats._fields_] == list(STATS_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_map_gated.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vgicp_gated_insert_stats));\n' +
                   "".join(f'  printf(" %zu", offsetof(vgicp_gated_insert_stats, {f}));\n' for f in STATS_FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [64] + [getattr(capi.GatedInsertStats, f).offset for f in STATS_FIELDS]
    assert got[1:] == [0, 8, 16, 24, 32, 40, 44, 48, 56]


def test_entry_points_refuse_a_null_context_and_a_foreign_one_and_write_nothing():
    lib = capi.load_library()
    pose = (C.c_double * 16)(*np.eye(4).reshape(16))
    stats = capi.GatedInsertStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    before = bytes(stats)
    kept = (C.c_uint8 * 8)(*([0xA5] * 8))
    points, refused = C.c_uint64(7), C.c_uint64(7)
    foreign = C.create_string_buffer(4096)       # a block that no build of the module stamped
    for ctx in (None, C.cast(foreign, C.c_void_p)):
        assert lib.vgicp_map_insert_resident_gated(ctx, pose, 20, 0.04, 8, kept, C.byref(stats)) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_map_insert_resident_gated_async(ctx, pose, 20, 0.04) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_map_gated_totals(ctx, C.byref(points), C.byref(refused)) == capi.ERR_BAD_ARGUMENT
        if ctx is not None:
            assert "not from one build" in lib.vgicp_last_error(None).decode()
    assert bytes(stats) == before and bytes(kept) == b"\xa5" * 8 and (points.value, refused.value) == (7, 7)
    assert foreign.raw == bytes(4096)


# ---- the host plans ---------------------------------------------------------------------------------------------------
def native(tmp_path, name, include, *args):
    exe = tmp_path / name
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + include, "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", name + ".cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    return run.stdout


# sha256 of `map_gated_plan list` built against the header of the commit before the gated entries: one line per (old
# entry, facts) with status, nothing-to-do and text
OLD_VERDICTS = "d12c28f879e2e027dc433072c5ae29701c01c81a6e13a85b516db96825fee4ac"


def test_insert_plan_of_the_gated_entries(tmp_path):
    """tests/native/map_gated_plan.cpp: plan_insert gives the gated entries the resident entries' verdicts over every
    combination of the facts, the four entries from before keep theirs (their listing hashes to what it hashed to before),
    and plan_gate applies rules 4 to 7 in the header's order."""
    csrc = os.path.join(ROOT, "eskf_lio_amd", "csrc")
    assert native(tmp_path, "map_gated_plan", csrc).strip() == \
        "ok 1024 verdicts (984 refused, 10 nothing to do), 144 gate checks"
    listing = native(tmp_path, "map_gated_plan", csrc, "list")
    assert len(listing.splitlines()) == 4 * 32 * 4 * 4
    assert hashlib.sha256(listing.encode()).hexdigest() == OLD_VERDICTS
    assert native(tmp_path, "map_plan", csrc).startswith("ok ")       # and against its own restatement, as before


def test_shim_plan_with_a_gate(tmp_path):
    """tests/native/update_plan_gated.cpp: with a gate the resident route uses the gated entry and a host-cloud frame is
    plain and counted; without one the plan is today's, field by field.  The raw points of a gated map are on the device:
    setInsertGate switches the store on (or refuses), and save() reads it."""
    out = native(tmp_path, "update_plan_gated", os.path.join(ROOT, "include"))
    assert out.strip() == "ok 512 plans, 256 through the gated entry, 112 plain frames counted"
    assert native(tmp_path, "update_plan", os.path.join(ROOT, "include")).startswith("ok ")
    shim = open(os.path.join(ROOT, "include", "eskf_lio_shim", "LocalMap.hpp")).read()
    for name in ("setInsertGate", "insertGate()", "gatedTotals()", 'm["insert_gate"]', "vgicp_map_insert_resident_gated_async",
                 "plan.entry == Plan::Entry::Gated", "plan.countPlain", "rawOnDevice_ = true"):
        assert name in shim, name


def test_replay_flag_parses_and_the_oracle_backend_refuses_it(oracle):
    src = open(os.path.join(ROOT, "tools", "replay.py")).read()
    assert '"--insert-gate"' in src and "insert_gate=args.insert_gate" in src
    from eskf_lio_amd import replay
    from replay_backends import OracleBackend
    assert "insert_gate" not in replay.DEFAULT_CONFIG["local_map"] and replay.insert_gate_of(replay.DEFAULT_CONFIG) == 0.0
    gated = dict(replay.DEFAULT_CONFIG, local_map=dict(replay.DEFAULT_CONFIG["local_map"], insert_gate=0.04))
    assert replay.insert_gate_of(gated) == 0.04
    replay.Odometry(replay.DEFAULT_CONFIG, OracleBackend(replay.DEFAULT_CONFIG, oracle))       # without the key: as before
    with pytest.raises(ValueError, match="local_map.insert_gate needs a backend"):
        replay.Odometry(gated, OracleBackend(gated, oracle))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="insert_gate must be"):
            replay.insert_gate_of(dict(gated, local_map=dict(gated["local_map"], insert_gate=bad)))
    assert replay.DeviceBackend.supports_insert_gate and not replay.GpuBackend.supports_insert_gate
    # refused where the gate could not be applied, before any context is made: the host-class backend (it hands the map
    # a host cloud every frame) and a multi-device context
    for make in (lambda: replay.GpuBackend(gated, device_resident_map=True), lambda: replay.DeviceBackend(gated, [0, 0])):
        with pytest.raises(ValueError, match="local_map.insert_gate needs"):
            make()
    # the command line: the flag needs a device map, and reaches the configuration
    tool = os.path.join(ROOT, "tools", "replay.py")
    for extra in ([], ["--device-map"]):
        run = subprocess.run(["python", tool, "--synthetic", "1", "--insert-gate", "0.04", *extra], capture_output=True, text=True)
        assert run.returncode == 2 and "--insert-gate needs --resident" in run.stderr
    run = subprocess.run(["python", tool, "--synthetic", "1", "--insert-gate", "0.04"], capture_output=True, text=True)
    assert run.returncode == 2 and "--insert-gate needs --resident" in run.stderr
    assert "--insert-gate" in subprocess.run(["python", tool, "--help"], capture_output=True, text=True, check=True).stdout


# ---- the rule ----------------------------------------------------------------------------------------------------------
def test_rule_restatement():
    inf, nan = float("inf"), float("nan")
    d2 = np.array([0.01, 0.05, -0.3, nan, inf, inf, 0.0])
    status = np.array([1, 1, 1 | 2, 1 | 4, 1 | 4, 0, 1], dtype=np.uint8)
    assert mg.rule(d2, status, 0.04).tolist() == [1, 0, 1, 0, 0, 1, 1]
    assert mg.rule(d2, status, 0.0).tolist() == [0, 0, 1, 0, 0, 1, 1]
    assert mg.rule(d2, status, inf).tolist() == [1, 1, 1, 0, 0, 1, 1]          # not finite: refused at every gate
    assert mg.counts(status, mg.rule(d2, status, 0.04)) == (6, 3, 2)


# ---- preconditions of tests/test_map_gated.py, on the reference alone ------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle):
    vmap, pts, covs, T_true, guess = rr.make_scene()
    om = oracle.OracleMap(vmap.voxel_size, 20)
    p, c, T = mg.first_scan(vmap)
    om.insert(*oracle.transform(p, c, T))
    return vmap, om, pts, covs, T_true


def test_scene_built_by_insertion_is_the_scene_and_both_classes_exist(scene, oracle):
    """The map built by inserting first_scan holds vmap's voxels bit for bit (count 1), so the scene's d^2 are those of
    tests/test_points_cpu.py: no gate of GATES within 1e-9 of a d^2 (the device's bound is 8e-11), and at 0.04 both
    classes are non-empty."""
    vmap, om, pts, covs, T_true = scene
    k, m, c, n = mg.sorted_oracle_export(om)
    order = np.lexsort(vmap.keys.T)
    assert np.array_equal(k, vmap.keys[order]) and m.tobytes() == vmap.means[order].tobytes()
    assert c.tobytes() == vmap.covs[order].tobytes() and np.all(n == 1)
    ref = pr.reference_at(oracle, om, pts, covs, T_true)
    assert len(ref.index) == 5856 and np.isfinite(ref.raw).all() and (ref.raw > 0.0).all()
    assert min(pr.gate_margin(ref.raw, g) for g in pr.GATES) > 1e-9
    inside = int(np.count_nonzero(ref.raw <= 0.04))
    assert 0 < inside < len(ref.index)
    print(f"at 0.04: {inside} matched points kept, {len(ref.index) - inside} refused, {6000 - len(ref.index)} unmatched")


def test_lists_scene_fills_lists_beyond_one_chunk(oracle):
    """The prepared pair: with the 0.9 quantile of d^2 as the gate, some voxel of the 0.3 m map still receives more than
    kListChunk kept points, for each max_points_per_voxel of the GPU test."""
    raw_a, raw_b = mg.lidar_pair()
    pa, ca, _ = oracle.preprocess(raw_a, mg.PREP_VOXEL, 30)
    pb, cb, _ = oracle.preprocess(raw_b, mg.PREP_VOXEL, 30)
    for cap in (1, 2, 20):
        om = oracle.OracleMap(mg.MAP_VOXEL, cap)
        om.insert(pa, ca)
        ref = pr.reference_at(oracle, om, pb, cb, np.eye(4))
        gate = pr.order_statistics(ref.ranked, [0.9])[0]
        d2, status = np.full(len(pb), np.inf), np.zeros(len(pb), dtype=np.uint8)
        d2[ref.index], status[ref.index] = ref.raw, pr.MATCHED
        kept = mg.rule(d2, status, gate).astype(bool)
        assert 0 < int((~kept).sum()) < len(ref.index) < len(pb)
        assert mg.per_voxel_counts(pb[kept], mg.MAP_VOXEL).max() > mg.LIST_CHUNK


def test_crafted_voxel_alternates(oracle):
    """Test 3's twelve points: all in voxel (0, 0, 0), in twelve cells of the 0.1 m grid (the preparation keeps them, in
    order), alternately a factor of ten inside and outside the gate of either route."""
    first, first_c, pts, covs = mg.crafted_voxel()
    assert not np.floor(pts[:12] / mg.MAP_VOXEL).any() and not np.floor(first / mg.MAP_VOXEL).any()
    assert len(np.unique(np.floor(pts[:12] / mg.PREP_VOXEL), axis=0)) == 12
    assert np.floor(pts[12:] / mg.MAP_VOXEL).any(axis=1).all()
    om = oracle.OracleMap(mg.MAP_VOXEL, 20)
    om.insert(first, first_c)
    prepared, prepared_c, _ = oracle.preprocess(pts, mg.PREP_VOXEL, 30)
    assert prepared[:12].tobytes() == pts[:12].tobytes()
    for gate, (p, c) in ((1.0, (pts, covs)), (0.02, (prepared, prepared_c))):
        ref = pr.reference_at(oracle, om, p, c, np.eye(4))
        assert ref.index.tolist() == list(range(12))
        assert (ref.raw[0::2] < gate / 10.0).all() and (ref.raw[1::2] > gate * 10.0).all(), ref.raw


def test_chain_preconditions(oracle):
    """Test 9's chain on the oracle: every displaced point lands in a voxel the map already holds; the gate separates the
    classes on the reference alone (static matched points at most gate / 2, displaced ones at least 2 gate, so
    gate_margin >= 0.5 against the device's 8e-11); both classes are there in every frame; and the displaced points, had
    they been inserted, would have changed the map."""
    from eskf_lio_amd import synth
    vmap = synth.make_map(20_000)
    frames, om = mg.make_chain(oracle, vmap)
    assert len(frames) == mg.CHAIN_FRAMES
    walk = oracle.OracleMap(vmap.voxel_size, mg.CHAIN_CAP)
    plain = oracle.OracleMap(vmap.voxel_size, mg.CHAIN_CAP)
    for m in (walk, plain):
        m.insert(*mg.first_scan(vmap)[:2])
    for pts, covs, T, moved, raw in frames:
        ref = pr.reference_at(oracle, walk, pts, covs, T)
        matched = np.zeros(len(pts), dtype=bool)
        matched[ref.index] = True
        assert matched[moved].all() and 100 < int(moved.sum()) < int((~moved).sum())
        d2 = np.full(len(pts), np.inf)
        d2[ref.index] = ref.raw
        assert (d2[moved] >= 2.0 * mg.CHAIN_GATE).all() and (d2[~moved & matched] <= 0.5 * mg.CHAIN_GATE).all()
        assert pr.gate_margin(ref.raw, mg.CHAIN_GATE) >= 0.5 and ref.raw.tobytes() == raw.tobytes()
        status = matched.astype(np.uint8)
        assert np.array_equal(mg.rule(d2, status, mg.CHAIN_GATE), (~moved).astype(np.uint8))
        walk.insert(*oracle.transform(pts[~moved], covs[~moved], T))
        plain.insert(*oracle.transform(pts, covs, T))
    a, b, c = mg.sorted_oracle_export(walk), mg.sorted_oracle_export(om), mg.sorted_oracle_export(plain)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert np.array_equal(a[0], c[0]) and a[1].tobytes() != c[1].tobytes()
