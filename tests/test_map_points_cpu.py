"""The raw-point extension of the C ABI (include/vgicp_hip_map_points.h) without a device: the library exports what the
extension header declares, the entry points refuse a NULL context, and the main header's pinned list is untouched."""
import os
import re

from eskf_lio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(vgicp_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_the_extension_header():
    lib = capi.load_library()
    names = declared("vgicp_hip_map_points.h")
    assert names == sorted(capi.MAP_POINTS_EXPORTS) == ["vgicp_map_points_export", "vgicp_map_points_size"]
    for name in names:
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_points.h")).read()
    assert re.search(r"#define\s+VGICP_OPTION_MAP_RAW_POINTS\s+4\b", text)
    assert '#include "vgicp_hip.h"' in text
    assert capi.OPTION_MAP_RAW_POINTS == 4


def test_extension_rejects_a_null_context():
    import ctypes as C
    lib = capi.load_library()
    p, c, w = C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
    assert lib.vgicp_map_points_size(None, C.byref(p), C.byref(c)) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_map_points_size(None, None, None) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_map_points_export(None, 0, None, None, C.byref(w)) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_set_option(None, capi.OPTION_MAP_RAW_POINTS, 1) == capi.ERR_BAD_ARGUMENT
    assert p.value == 7 and c.value == 7


def test_main_header_keeps_its_47_entry_points():
    names = declared("vgicp_hip.h")
    assert len(names) == 47
    assert sorted(capi.EXPORTS) == names
    assert not set(names) & set(capi.MAP_POINTS_EXPORTS)
    assert capi.load_library().vgicp_abi_version() == 6
