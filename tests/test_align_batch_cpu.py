"""The batched align's extension of the C ABI (include/vgicp_hip_batch.h) without a device: the library exports what the
extension header declares, the Python mirror of vgicp_batch_stats has the header's layout, the entry points refuse a
NULL context, and the main header's pinned list is untouched."""
import ctypes as C
import os
import re
import subprocess

from eskf_lio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("hypotheses_per_launch", "launches", "seconds", "device_seconds", "status", "iterations", "converged",
          "corr_count", "normal_eq")


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(vgicp_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_the_batch_header():
    lib = capi.load_library()
    names = declared("vgicp_hip_batch.h")
    assert names == sorted(capi.BATCH_EXPORTS) == ["vgicp_align_batch_width", "vgicp_align_resident_batch"]
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    for name in names:
        assert name in exported and hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "vgicp_hip_batch.h")).read()
    assert '#include "vgicp_hip.h"' in text
    assert re.search(r"#define\s+VGICP_BATCH_MAX\s+64\b", text) and capi.BATCH_MAX == 64
    # the main header's pinned list is untouched, and so is the ABI version
    main = declared("vgicp_hip.h")
    assert len(main) == 47 and sorted(capi.EXPORTS) == main
    assert not set(main) & set(capi.BATCH_EXPORTS) and not set(capi.MAP_POINTS_EXPORTS) & set(capi.BATCH_EXPORTS)
    assert lib.vgicp_abi_version() == 6


def test_batch_stats_layout_matches_the_header(tmp_path):
    # pinned (LP64): two int32, two doubles, five pointers
    assert C.sizeof(capi.BatchStats) == 64
    want = dict(hypotheses_per_launch=0, launches=4, seconds=8, device_seconds=16, status=24, iterations=32,
                converged=40, corr_count=48, normal_eq=56)
    assert [f for f, _ in capi.BatchStats._fields_] == list(FIELDS)
    for name, off in want.items():
        assert getattr(capi.BatchStats, name).offset == off, name
    # ... and what the C compiler makes of the header itself
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_batch.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vgicp_batch_stats));\n' +
                   "".join(f'  printf(" %zu", offsetof(vgicp_batch_stats, {f}));\n' for f in FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.BatchStats)] + [getattr(capi.BatchStats, f).offset for f in FIELDS]


def test_batch_entry_points_reject_a_null_context():
    lib = capi.load_library()
    g, out = (C.c_double * 16)(), (C.c_double * 16)()
    p = capi.Params(5, 0, 1e-6, 0.9999, 0, 0)
    st = capi.BatchStats()
    st.hypotheses_per_launch = 7
    w = C.c_size_t(7)
    assert lib.vgicp_align_resident_batch(None, 1, g, C.byref(p), out, C.byref(st)) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_align_resident_batch(None, 0, None, None, None, None) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_align_batch_width(None, C.byref(w)) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_align_batch_width(None, None) == capi.ERR_BAD_ARGUMENT
    assert st.hypotheses_per_launch == 7 and w.value == 7
