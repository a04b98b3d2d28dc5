"""What a map update decides before it touches the device — the first table and raw-point log, when and how far they grow,
whether an insertion goes without its sort, what each insertion entry refuses — are pure functions
(eskf_lio_amd/csrc/vgicp_map_plan.h): checked on the CPU, without a device, against the hand-written predicates they
replaced.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_plan_reproduces_the_hand_written_predicates(tmp_path):
    """tests/native/map_plan.cpp restates vgicp_map_reset's, raw_reset's, ensure_table's and ensure_raw's arithmetic,
    insertion_lists_stay_short and the checks of the four insertion entries as they stood, and compares every field of
    every plan with them:
    first sizes — capacity hints whose fourfold lies on and one past 1024 slots / 4096 entries, 2^31 entries, 2^32 slots (10);
    table growth — slots in {none, 1024, 2^20, 2^32} x (the load at slots / 2 and one past, carried by voxels, incoming,
    tombstones and the pending insertion's bound in turn; (voxels + incoming) x 4 at 2^32 and one past, carried by either) (48);
    raw-point log — capacity in {4096, 2^20, 2^31} x (2 (live + n) at the capacity and one point past, live + n at 2^31 and
    one past; used + n at the capacity and one past), each as one more point and as all points incoming (36);
    short lists — map voxel / scan voxel in {1, 2, 3, 3 + one ulp, 4} at two scan voxels, scan voxel 0, negative and NaN,
    each with insert_sort off and on (26);
    insertion verdict — the four entries x every combination of the five boolean facts x n in {0, 1, 2^31 - 1, 2^31} x
    points per voxel in {0, 1, 2^32 - 1, 2^32} (2048).
    Nothing is skipped: the program counts what it visited, and every outcome — both "too large" refusals and "nothing to
    do" among them — must have been planned at least once."""
    exe = tmp_path / "map_plan"
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "map_plan.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-500:]
    words = run.stdout.split()
    checks = 10 + 4 * (2 * 4 + 2 * 2) + 3 * (4 * 2 + 2 * 2) + (2 * 5 + 3) * 2 + 4 * 2 ** 5 * 4 * 4
    assert words[0] == "ok" and int(words[1]) == checks == 2168, run.stdout
    counts = dict(zip(words[3::2], map(int, words[4::2])))
    tables = {"table-kept", "table-grown", "table-too-large"}
    growths, fills = {"raw-same-size", "raw-grown", "raw-too-large"}, {"raw-fits", "raw-compacted"}
    lists = {"short-lists", "sorted"}
    verdicts = {"insert", "nothing-to-do", "no-map", "no-scan", "null-pointer", "cap-zero", "cap-raw", "shard", "scan-too-large"}
    assert set(counts) == tables | growths | fills | lists | verdicts and all(v > 0 for v in counts.values()), run.stdout
    assert [sum(counts[k] for k in group) for group in (tables, growths, fills, lists, verdicts)] == [58, 24, 12, 26, 2048]
