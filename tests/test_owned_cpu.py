"""The context holds its device memory, page-locked memory, events and stream in the move-only owners of
eskf_lio_amd/csrc/vgicp_owned.h.  tests/native/owned.cpp drives them over a counting backend on the CPU: what a regrow
frees and when, what a failed allocation leaves behind, moves, release(), the device alias of page-locked memory, and
the shape of a context's creation that fails half way.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 4 cases for each of the two buffer owners, 1 for untyped memory, 8 + 1 for the struct of eight owners (allocation k
# fails, k = 1 .. 8; none fails), 1 each for the alias, the events and the stream
CASES = 2 * 4 + 1 + 8 + 1 + 3


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_owners_free_once_in_order_and_leave_nothing_after_a_failure(tmp_path, sanitize):
    """Allocate then regrow: the old block is freed exactly once, before the new allocation is requested.  A failed
    regrow leaves the owner empty and nothing live.  Move construction and assignment (onto a non-empty owner, onto
    itself), release(), eight owners filled in order with allocation k failing for every k, the alias requested once and
    cleared by reset(), events created, destroyed and reset twice.  The second build runs the same program under the
    address and undefined-behaviour sanitizers (host code only): a double free or a use after a move ends it."""
    exe = tmp_path / "owned"
    # the sanitizers' runtimes linked in: the program then runs whatever else the environment preloads
    flags = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
             if sanitize else ["-O2"])
    out = subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror",
                          "-I" + os.path.join(ROOT, "eskf_lio_amd", "csrc"), "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "owned.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) == CASES == 21, run.stdout
