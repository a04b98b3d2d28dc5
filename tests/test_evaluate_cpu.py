"""The evaluation's extension of the C ABI (include/vgicp_hip_evaluate.h) without a device: the library exports what the
extension header declares, the Python mirror of vgicp_evaluation has the header's layout, the entry point refuses a
NULL context, the main header's pinned list is untouched, and the drop-in's choice by score picks what its rule says
on hand-made values."""
import ctypes as C
import os
import re
import subprocess

from eskf_lio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("points", "correspondences", "cost", "sq_error", "normal_eq")
STATS_FIELDS = ("launches", "poses_per_launch", "seconds", "device_seconds")


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(vgicp_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_the_evaluate_header():
    lib = capi.load_library()
    names = declared("vgicp_hip_evaluate.h")
    assert names == sorted(capi.EVALUATE_EXPORTS) == ["vgicp_evaluate_resident"]
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    for name in names:
        assert name in exported and hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "vgicp_hip_evaluate.h")).read()
    assert '#include "vgicp_hip.h"' in text
    assert re.search(r"#define\s+VGICP_EVAL_MAX\s+64\b", text) and capi.EVAL_MAX == 64
    # the main header's pinned list is untouched, so are the other extension headers' and the ABI version
    main = declared("vgicp_hip.h")
    assert len(main) == 47 and sorted(capi.EXPORTS) == main
    others = set(main) | set(capi.MAP_POINTS_EXPORTS) | set(capi.BATCH_EXPORTS)
    assert len(others) == 47 + 2 + 2 and not others & set(capi.EVALUATE_EXPORTS)
    assert declared("vgicp_hip_batch.h") == sorted(capi.BATCH_EXPORTS)
    assert declared("vgicp_hip_map_points.h") == sorted(capi.MAP_POINTS_EXPORTS)
    assert exported == others | set(capi.EVALUATE_EXPORTS)     # the library exports exactly the four lists
    assert lib.vgicp_abi_version() == 6


def test_evaluation_layout_matches_the_header(tmp_path):
    # pinned (LP64): two uint64, two doubles, 27 doubles
    assert C.sizeof(capi.Evaluation) == 248
    want = dict(points=0, correspondences=8, cost=16, sq_error=24, normal_eq=32)
    assert [f for f, _ in capi.Evaluation._fields_] == list(FIELDS)
    for name, off in want.items():
        assert getattr(capi.Evaluation, name).offset == off, name
    assert C.sizeof(capi.EvalStats) == 24 and [f for f, _ in capi.EvalStats._fields_] == list(STATS_FIELDS)
    # ... and what the C compiler makes of the header itself
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_evaluate.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vgicp_evaluation));\n' +
                   "".join(f'  printf(" %zu", offsetof(vgicp_evaluation, {f}));\n' for f in FIELDS) +
                   '  printf(" %zu", sizeof(vgicp_eval_stats));\n' +
                   "".join(f'  printf(" %zu", offsetof(vgicp_eval_stats, {f}));\n' for f in STATS_FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == ([248] + [getattr(capi.Evaluation, f).offset for f in FIELDS] +
                   [C.sizeof(capi.EvalStats)] + [getattr(capi.EvalStats, f).offset for f in STATS_FIELDS])


def test_evaluate_rejects_a_null_context_and_writes_nothing():
    lib = capi.load_library()
    poses = (C.c_double * 32)(*([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0] * 2))
    out = (capi.Evaluation * 2)()
    C.memset(out, 0xA5, C.sizeof(out))
    before = bytes(out)
    st = capi.EvalStats()
    st.launches, st.poses_per_launch = 7, 9
    assert lib.vgicp_evaluate_resident(None, 2, poses, out, C.byref(st)) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_evaluate_resident(None, 0, None, None, None) == capi.ERR_BAD_ARGUMENT
    assert bytes(out) == before and (st.launches, st.poses_per_launch) == (7, 9)


def test_pose_evaluation_derives_fitness_and_rmse():
    e = capi.PoseEvaluation(points=1000, correspondences=800, cost=100.0, sq_error=8.0, normal_eq=np_row())
    assert e.fitness == 0.8 and e.inlier_rmse == 0.1
    assert e.JTJ.shape == (6, 6) and (e.JTJ == e.JTJ.T).all() and e.JTJ[5, 5] == 21.0 and e.JTJ[1, 0] == 2.0
    assert list(e.JTr) == [22.0, 23.0, 24.0, 25.0, 26.0, 27.0]
    none = capi.PoseEvaluation(points=1000, correspondences=0, cost=0.0, sq_error=0.0, normal_eq=np_row())
    assert none.fitness == 0.0 and none.inlier_rmse == 0.0


def np_row():
    import numpy as np
    return np.arange(1.0, 28.0)


def test_shim_select_best_by_score_on_hand_made_values(tmp_path):
    """tests/native/shim_score.cpp against the stand-in types: Evaluation::fitness / inlierRmse / score / information,
    and selectBestByScore — converged before unconverged, a fuller match beats a lower cost per match, ties to the
    lower index."""
    exe = tmp_path / "shim_score"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                          "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_score.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout[-1000:] + run.stderr[-500:]
