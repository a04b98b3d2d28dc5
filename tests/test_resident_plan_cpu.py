"""The calls over the resident scan at a pose without a device: what vgicp_evaluate_resident and
vgicp_align_resident_batch refuse (eskf_lio_amd/csrc/vgicp_resident_plan.h), the layout of the argument structs that
begin with the pose view, and that the pieces these entries share are written once (vgicp_capi_resident.inl)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eskf_lio_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_resident_plan(tmp_path):
    """tests/native/resident_plan.cpp: plan_evaluate and plan_batch over every combination of their facts against the
    ordered lists and every text; sizeof / offsetof of PoseView, PointArgs and GateArgs (vgicp_device.h compiled for the
    host alone)."""
    exe = tmp_path / "resident_plan"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                          "-isystem", os.path.join(ROCM, "include"), "-I" + CSRC, "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "resident_plan.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    assert run.stdout.splitlines() == ["evaluate ok %d" % (128 * 4 * 4), "batch ok %d" % (512 * 4 * 3), "layout ok 152 224 176"]


def source(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_shared_pieces_are_written_once():
    entries = ["vgicp_capi_batch.inl", "vgicp_capi_evaluate.inl", "vgicp_capi_points.inl", "vgicp_capi_map_gated.inl"]
    frame = source("vgicp_capi_resident.inl")
    # "this context has several devices", the timed span's read-out and the readiness texts
    assert frame.count("peers_connected") == 1 and frame.count("hipEventElapsedTime") == 1
    for name in entries:
        text = source(name)
        assert "hipEventElapsedTime" not in text and "now_seconds() - t0" not in text, name
        if name != "vgicp_capi_batch.inl":
            assert "peers_connected" not in text, name
    for name in ("vgicp_capi_evaluate.inl", "vgicp_capi_batch.inl"):
        assert "no voxel map" not in source(name) and "no scan resident" not in source(name), name
    # the layout handshake: one comparison and one function that refuses by it, in vgicp_context.h, used by every
    # library beside the module (the Makefile's list)
    sources = [f for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".inl"))]
    assert sum(len(re.findall(r"kLayoutMark \|", source(f))) for f in sources) == 2          # the stamp and same_build
    assert len(re.findall(r"same_build\(ctx\)", source("vgicp_context.h"))) == 1             # in layout_handshake
    side = re.search(r"^SIDE := (.+)$", source("Makefile"), re.M).group(1).split()
    assert len(side) >= 8 and {"prior", "points", "map_locate"} <= set(side)
    for lib in ("vgicp_%s.hip" % name for name in side):
        text = source(lib)
        assert "VG_RC(layout_handshake(ctx, " in text or "same_build(ctx)" in text, lib
        assert "kLayoutMark" not in text and not re.search(r"\bhandshake\s*\([^;{]*\)\s*\{", text), lib
    # the ray walk of carving and of the ray report: the step's comparison and the step bound's cap, once each
    everything = "".join(source(f) for f in sources)
    assert everything.count("tx <= ty && tx <= tz") == 1 and everything.count("4097.0") == 1
