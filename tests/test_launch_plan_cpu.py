"""Which instantiation of a round kernel a launch takes is ONE pure function per launcher
(eskf_lio_amd/csrc/vgicp_launch_plan.h: plan_iterate, plan_close, plan_persistent) over ONE list of instantiations each:
checked on the CPU, without a device, against the hand-written launchers they replaced.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_reproduces_the_hand_written_launchers(tmp_path):
    """tests/native/launch_plan.cpp enumerates every combination of the boolean facts (robust kernel, gate, prior, stamps,
    world in {1, 2}), block in {128, 256, 512, 1024}, n in {0, 1, 448 grid, 448 grid + 1} for grid in {1, 2, 256},
    memo_points in {0, 3, 19}, stash_bytes in {0, 100 000, 200 000}, prefetch_margin in {0, 0.015}, and compares the
    refusal, or the flags of the chosen instantiation and the dynamic LDS size, with launch_iterate (+
    launch_iterate_prior), launch_close and launch_persistent as they stood before.  No list has a duplicate, every
    entry is reached, every accepted fact has exactly one entry; the program counts what it visited."""
    exe = tmp_path / "launch_plan"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "launch_plan.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    words = run.stdout.split()
    combinations = 2 * 4 * 2 * 2 * 2 + 2 * 2 * 3 * 4 * 3 * 3 * 2 * 2 * 2 * 2
    assert words[0] == "ok" and int(words[1]) == combinations == 6_976, run.stdout
    counts = dict(zip(words[3::2], map(int, words[4::2])))
    assert counts["iterate"] == 12 and counts["close"] == 6 and counts["persistent"] == 14, run.stdout
    assert 0 < counts["refused"] < combinations
