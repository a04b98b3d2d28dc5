"""Which host path an align takes is ONE pure function (eskf_lio_amd/csrc/vgicp_align_plan.h: plan_align): checked on the
CPU, without a device, against the hand-written predicates it replaced.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_plan_reproduces_the_hand_written_predicates(tmp_path):
    """tests/native/align_plan.cpp enumerates every combination of the boolean facts (13 of them), n in {0, 1, 448, 449,
    grid * 448, grid * 448 + 1}, grid in {8, 122, 256}, cool-down in {0, 1, 8}, max_iteration in {0, 1, 63, 64}, k in
    {1, 2, 16}, world sizes {1, 2}, for each of the four calls (vgicp_align, vgicp_align_resident, the batch, a
    multi-device group), and compares path, cool-down step, peer path, team width and workgroups per team with the five
    predicates as they stood before (fused_align_fits, run_align's single_launch, batch_width + wide, the
    one-point-per-thread test, align_shards' single).  Nothing is skipped: the program counts what it visited, and every
    AlignPath must have been planned at least once."""
    exe = tmp_path / "align_plan"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "align_plan.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    words = run.stdout.split()
    combinations = 4 * 3 * 6 * 3 * 4 * 3 * 2 * 2 * 2 ** 13
    assert words[0] == "ok" and int(words[1]) == combinations == 84_934_656, run.stdout
    counts = dict(zip(words[3::2], map(int, words[4::2])))
    assert set(counts) == {"fused", "persistent", "teams", "loop", "group-loop"} and all(v > 0 for v in counts.values())
    assert sum(counts.values()) == combinations
