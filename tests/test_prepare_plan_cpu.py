"""How a scan preparation's raw sweep reaches the device is ONE pure function (eskf_lio_amd/csrc/vgicp_prepare_plan.h:
plan_prepare): checked on the CPU, without a device, against the hand-written predicates it replaced.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prepare_plan_reproduces_the_hand_written_predicates(tmp_path):
    """tests/native/prepare_plan.cpp enumerates ahead, with_deskew, ordered, bounds_fused in {0, 1}, used in {1, 4096, 4097,
    16000}, n in {1, 524 288, 524 289, 699 050, 699 051} (n * 32 and n * 24 bytes exactly on and one point past the 16 MB
    default) and stage_limit in {0, 1, 16 MB, SIZE_MAX}, and compares every field of the plan — route, walk, times by unit,
    times by the calling thread, time source, time copy, the state-table slot's event and the in-place route's wait — with
    scan_prepare_enqueue's predicates as they stood before.  Nothing is skipped: the program counts what it visited, and
    every route and every time source must have been planned at least once."""
    exe = tmp_path / "prepare_plan"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "prepare_plan.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    words = run.stdout.replace("|", " ").split()
    combinations = 2 ** 4 * 4 * 5 * 4
    assert words[0] == "ok" and int(words[1]) == combinations == 1280, run.stdout
    counts = dict(zip(words[3::2], map(int, words[4::2])))
    routes, sources = {"ahead", "staged", "in-place"}, {"none", "ahead-slot", "staged-times", "device"}
    assert set(counts) == routes | sources and all(v > 0 for v in counts.values()), run.stdout
    assert sum(counts[k] for k in routes) == combinations == sum(counts[k] for k in sources)
