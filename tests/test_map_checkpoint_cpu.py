"""The map checkpoint (include/vgicp_hip_map_checkpoint.h) without a device: the numpy restatement of the blob on hand-made
blobs and the formula, the plan header's check enumerated by a native program (plain, and under the address and undefined
behaviour sanitizers as a stand-alone program), the two checks held against each other on the same mutated blobs, the
header against the Python mirror and the Makefile, the host-only entry point, and the shim's file round trip on a stand-in
of the C ABI."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import map_checkpoint_reference as mc
from eskf_lio_amd import capi
from test_evaluate_cpu import declared
from test_map_gated_cpu import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eskf_lio_amd", "csrc")
INFO_FIELDS = ("format", "header_bytes", "total_bytes", "voxel_size", "slots", "voxels", "tombstones", "raw_points", "flags",
               "record_bytes", "checksum", "rule", "reserved")
STATS_FIELDS = ("bytes", "voxels", "tombstones", "raw_points", "launches", "reserved", "seconds", "device_seconds")


def small_blob(F=3, T=2, raw=True, slots=1024):
    keys = np.stack([np.arange(F), -np.arange(F), np.full(F, 7)], axis=1).astype(np.int32)
    means = (keys + 0.5) * 0.5
    covs = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 3.0]) * 0.01, (F, 1))
    counts = 1 + np.arange(F, dtype=np.uint64) % 3
    pts = np.arange(3 * int(counts.sum()), dtype=np.float64).reshape(-1, 3) * 0.125 if raw else None
    return mc.pack(0.5, slots, 3 * np.arange(F) + 1, mc.records_of(keys, means, covs, counts), 3 * np.arange(T) + 2, pts)


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_the_formula_the_sections_and_the_header_of_hand_made_blobs():
    for F in (0, 1, 2, 64, 65):
        for T in (0, 1, 3):
            for raw in (False, True):
                blob = small_blob(F, T, raw)
                P = int((1 + np.arange(F) % 3).sum()) if raw else 0
                assert len(blob) == 128 + mc.pad8(4 * F) + mc.pad8(4 * T) + 128 * F + 24 * P == mc.total_bytes(F, T, P)
                assert len(blob) % 8 == 0 and mc.check(blob) == 0
                b = mc.parse(blob)
                h = b.header
                assert (h["magic"], h["format"], h["header_bytes"], h["record_bytes"]) == (b"VGICPMAP", 1, 128, 128)
                assert (h["total_bytes"], h["voxel_size"], h["slots"]) == (len(blob), 0.5, 1024)
                assert (h["voxels"], h["tombstones"], h["raw_points"], h["flags"]) == (F, T, P, int(raw))
                assert h["reserved"] == bytes(48) and h["checksum"] == mc.checksum(blob[128:])
                assert list(b.full_slots) == [3 * j + 1 for j in range(F)] and list(b.tomb_slots) == [3 * j + 2 for j in range(T)]
                assert (b.records["state"] == 1).all() and (b.records["spare"] == 0).all()
                assert [len(p) for p in b.raw_of_record()] == ([1 + j % 3 for j in range(F)] if raw else [0] * F)
    # the fields lie where the header says: read with struct, not with the restatement's own dtype
    blob = small_blob()
    assert struct.unpack_from("<8sIIQdQQQQIIQ", blob, 0) == (b"VGICPMAP", 1, 128, len(blob), 0.5, 1024, 3, 2, 6, 1, 128, mc.checksum(blob[128:]))
    assert blob[128 + 12:128 + 16] == bytes(4) and struct.unpack_from("<3I", blob, 128) == (1, 4, 7)        # the pad of an odd F
    assert struct.unpack_from("<2I", blob, 128 + 16) == (2, 5) and struct.unpack_from("<3iI", blob, 128 + 24) == (0, 0, 7, 1)
    assert struct.unpack_from("<QQ", blob, 128 + 24 + 112) == (1, 0) and struct.unpack_from("<3d", blob, 128 + 24 + 3 * 128) == (0.0, 0.125, 0.25)
    assert len(mc.pack(0.5, 1024, [], np.zeros(0, mc.RECORD_DTYPE))) == 128


def test_the_checksum_sees_every_flipped_bit_and_every_swap_of_unequal_words():
    words = np.array([5, 0, 2**63, 5, 2**64 - 1], dtype=np.uint64)
    want = (5 * 1 + 0 * 3 + 2**63 * 5 + 5 * 7 + (2**64 - 1) * 9) % 2**64
    assert mc.checksum(words.tobytes()) == want and mc.checksum(b"") == 0
    raw = bytearray(words.tobytes())
    for bit in range(8 * len(raw)):
        raw[bit // 8] ^= 1 << (bit % 8)
        assert mc.checksum(raw) != want, bit                # an odd factor is a unit mod 2^64
        raw[bit // 8] ^= 1 << (bit % 8)
    # words i and j swapped move the sum by (a - b) 2 (j - i) mod 2^64: nothing for equal words — and nothing either where
    # the difference ends in enough zero bits (2^63 one place apart), which is as far as a weighted sum goes
    for i in range(5):
        for j in range(i + 1, 5):
            w = words.copy()
            w[i], w[j] = words[j], words[i]
            moved = (int(words[i]) - int(words[j])) * 2 * (j - i) % 2**64 != 0
            assert (mc.checksum(w.tobytes()) != want) == moved, (i, j)
            assert moved == (words[i] != words[j]) or (i, j) == (1, 2)


# ---- the plan header's check ---------------------------------------------------------------------------------------------
def visited(out):
    assert out.startswith("ok ") and "MISMATCH" not in out, out
    counts = {int(r): int(c) for r, c in re.findall(r"rule (\d+) (\d+)", out)}
    assert sorted(counts) == list(range(1, 15)) and all(c > 0 for c in counts.values()), out          # every rule has fired
    n = {k: int(v) for k, v in re.findall(r"(built|mutations|truncations|flips|harmless|offered|passed) (\d+)", out)}
    assert n["built"] == 5 * 3 * 2 and n["mutations"] >= 14 and n["truncations"] > 128 and n["flips"] == 8 * n["truncations"]
    # what passes: the well-formed blobs, the five changes the check does not look at, and the flips of voxel_size that
    # leave it finite and > 0 (0.5: every bit but the sign), which the checksum does not cover
    assert n["harmless"] == 63 and n["passed"] == n["built"] + 5 + n["harmless"]
    return n


def test_the_check_fires_every_rule_and_lets_no_mutation_through(tmp_path):
    """tests/native/checkpoint_plan.cpp, and on the blobs it offered the restatement gives the same verdicts."""
    offered = tmp_path / "offered.bin"
    n = visited(native(tmp_path, "checkpoint_plan", CSRC, str(offered)).strip())
    data = offered.read_bytes()
    at, seen, by_rule = 0, 0, {}
    while at < len(data):
        size, rule = struct.unpack_from("<Ii", data, at)
        blob = data[at + 8:at + 8 + size]
        at += 8 + size
        seen += 1
        by_rule[rule] = by_rule.get(rule, 0) + 1
        assert mc.check(blob) == rule, (seen, rule, mc.check(blob))
    assert seen == n["offered"] and at == len(data) and sorted(by_rule) == list(range(15))


def test_the_check_is_clean_under_the_sanitizers(tmp_path):
    """The same program as a stand-alone g++ build with -fsanitize=address,undefined: nothing is loaded into Python."""
    exe = tmp_path / "checkpoint_plan_san"
    # the sanitizers' runtimes linked in (as tests/test_owned_cpu.py does): the program then runs whatever else the
    # environment preloads
    out = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC, "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "checkpoint_plan.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    visited(run.stdout.strip())


# ---- header, mirror, libraries ----------------------------------------------------------------------------------------------
def test_header_mirror_makefile_and_library_agree():
    lib = capi.load_library()
    names = ["vgicp_map_checkpoint", "vgicp_map_checkpoint_info", "vgicp_map_checkpoint_size", "vgicp_map_restore"]
    assert declared("vgicp_hip_map_checkpoint.h") == sorted(capi.MAP_CHECKPOINT_EXPORTS) == names
    assert capi.SIDE_EXPORTS["map_checkpoint"] is capi.MAP_CHECKPOINT_EXPORTS
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_checkpoint.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_map_checkpoint.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)           # no new vgicp_set_option number
    assert "`format` is bumped whenever either changes" in text and "SAFE to load, not necessarily meaningful" in text
    assert re.findall(r"^ \*\s+(\d+)\. ", text, flags=re.M)[:14] == [str(k) for k in range(1, 15)]          # the fourteen rules
    for macro, value in (("FORMAT", capi.CHECKPOINT_FORMAT), ("HEADER_BYTES", capi.CHECKPOINT_HEADER_BYTES), ("RECORD_BYTES", mc.RECORD),
                         ("RAW_POINTS", capi.CHECKPOINT_RAW_POINTS), ("RULES", capi.CHECKPOINT_RULES)):
        assert int(re.search(rf"#define\s+VGICP_CHECKPOINT_{macro}\s+(\d+)", text).group(1)) == value
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("map_checkpoint")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.MAP_CHECKPOINT_EXPORTS)
    assert all(hasattr(lib, name) for name in capi.MAP_CHECKPOINT_EXPORTS)
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    side = re.search(r"^SIDE := (.*)$", makefile, flags=re.M).group(1).split()
    assert "map_checkpoint" in side and set(side) == set(capi.SIDE_EXPORTS)
    assert makefile.count("vgicp_checkpoint_plan.h") >= 2 and "vgicp_capi_map_checkpoint.inl" in makefile
    # the module exports none of it: its list is still the main header's
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert exported == set(capi.EXPORTS + capi.MAP_POINTS_EXPORTS + capi.BATCH_EXPORTS + capi.EVALUATE_EXPORTS)
    assert lib.vgicp_abi_version() == 6 and "checkpoint" not in open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()
    # the kernels sit beside the submap's, the check in the plan header, which makes no HIP call
    plan = open(os.path.join(CSRC, "vgicp_checkpoint_plan.h")).read()
    assert "checkpoint_emit_kernel" in open(os.path.join(CSRC, "vgicp_mapupdate.hip")).read()
    assert "inline int checkpoint_check(" in plan and "hip_runtime" not in plan and "vgicp_context.h" not in plan


def test_struct_layouts_match_the_header(tmp_path):
    structs = (("vgicp_checkpoint_info", capi.CheckpointInfo, INFO_FIELDS, [80, 0, 4, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 76]),
               ("vgicp_checkpoint_stats", capi.CheckpointStats, STATS_FIELDS, [56, 0, 8, 16, 24, 32, 36, 40, 48]))
    body = ""
    for name, mirror, fields, _ in structs:
        assert [f for f, _ in mirror._fields_] == list(fields)
        body += f'  printf("%zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {f}));\n' for f in fields)
        body += '  printf("\\n");\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vgicp_hip_map_checkpoint.h"\nint main(void) {\n' + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    text = open(os.path.join(ROOT, "include", "vgicp_hip_map_checkpoint.h")).read()
    for line, (name, mirror, fields, want) in zip(lines, structs):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want, name
        assert re.search(rf"typedef struct {name} {{\s+/\* {want[0]} bytes, LP64", text), name          # the size is stated


def test_the_host_only_entry_reads_a_blob_and_names_the_rule():
    blob = small_blob()
    info = capi.map_checkpoint_info(blob)
    h = mc.parse(blob).header
    assert info["rule"] == 0 and info["message"] == ""
    assert all(info[k] == h[k] for k in INFO_FIELDS[:11])
    # a file as the shim writes it: the blob, then a trailer, read by total_bytes
    trailer = b"VGICPTRJ" + struct.pack("<Q", 0) + bytes(128)
    assert capi.map_checkpoint_info(blob + trailer)["rule"] == 0
    for change, rule in ((lambda b: b[:200], 8), (lambda b: b"XGICPMAP" + b[8:], 1), (lambda b: b[:300] + bytes([b[300] ^ 4]) + b[301:], 9),
                         (lambda b: b[:100], 1)):
        bad = change(blob)
        info = capi.map_checkpoint_info(bad)
        assert info["rule"] == rule == mc.check(bad) and f"rule {rule}:" in info["message"], (rule, info)
    lib = capi.load_library()
    raw = capi.CheckpointInfo()
    assert lib.vgicp_map_checkpoint_info(None, 128, C.byref(raw)) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_map_checkpoint_info(blob, len(blob), None) == capi.ERR_BAD_ARGUMENT


def test_the_entry_points_refuse_null_and_foreign_contexts_and_write_nothing():
    lib = capi.load_library()
    blob = small_blob()
    stats = capi.CheckpointStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    before = bytes(stats)
    foreign = C.create_string_buffer(4096)          # a block that no build of the module stamped
    f = C.cast(foreign, C.c_void_p)
    out = C.create_string_buffer(b"\x5a" * 256, 256)
    w = C.c_size_t(77)
    for ctx in (None, f):
        assert lib.vgicp_map_checkpoint_size(ctx, C.byref(w)) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_map_checkpoint(ctx, 256, out, C.byref(w), C.byref(stats)) == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_map_restore(ctx, blob, len(blob), C.byref(stats)) == capi.ERR_BAD_ARGUMENT
        text = lib.vgicp_last_error(None).decode()
        assert ("not from one build" in text) if ctx else ("NULL pointer" in text)
    assert lib.vgicp_map_checkpoint_size(f, None) == capi.ERR_BAD_ARGUMENT and "NULL pointer" in lib.vgicp_last_error(None).decode()
    assert lib.vgicp_map_checkpoint(f, 256, None, C.byref(w), None) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_map_checkpoint(f, 256, out, None, None) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_map_restore(f, None, 128, None) == capi.ERR_BAD_ARGUMENT
    assert bytes(stats) == before and w.value == 77 and out.raw == b"\x5a" * 256 and foreign.raw == bytes(4096)


# ---- the shim ----------------------------------------------------------------------------------------------------------------
def test_the_shim_writes_and_reads_a_checkpoint_file_on_a_stand_in_of_the_abi(tmp_path):
    """tests/native/shim_checkpoint.cpp links LocalMap.hpp against a stand-in of the C ABI whose map is a byte string: the
    file is the blob verbatim and the trailer, the blob comes back identical, the trajectory and prevTransform_ too, the
    file is written through path + ".tmp", and the shadow-grid modes refuse both methods."""
    exe = tmp_path / "shim_checkpoint"
    cmd = ["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-Wno-address", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "shim_checkpoint.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    path = tmp_path / "map.ckpt"
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1].startswith("ok "), run.stdout[-2000:] + run.stderr[-1000:]
    data = path.read_bytes()
    total = struct.unpack_from("<Q", data, 16)[0]
    assert data[:8] == b"VGICPMAP" and data[total:total + 8] == b"VGICPTRJ" and not os.path.exists(str(path) + ".tmp")
    n = struct.unpack_from("<Q", data, total + 8)[0]
    assert n == 4 and len(data) == total + 16 + 128 * (n + 1)
    poses = np.frombuffer(data, "<f8", 16 * (n + 1), total + 16).reshape(n + 1, 4, 4)
    assert [p[3, 0] for p in poses] == [1.0, 2.0, 3.0, 9.0, 9.0]          # column-major: the translations' x, then prevTransform_'s
    # Python reads such a file by total_bytes and ignores the trailer
    assert capi._blob_bytes(data).size == total
    lm = open(os.path.join(ROOT, "include", "eskf_lio_shim", "LocalMap.hpp")).read()
    for name in ("#pragma weak vgicp_map_checkpoint\n", "#pragma weak vgicp_map_restore\n", "void saveCheckpoint(const std::string & path)",
                 "void loadCheckpoint(const std::string & path)", "libvgicp_hip_map_checkpoint.so", '#include "../vgicp_hip_map_checkpoint.h"'):
        assert name in lm, name
    # no existing method's route has changed
    golden = open(os.path.join(ROOT, "tests", "golden", "shim_routes.txt")).read()
    assert "Checkpoint" not in golden
