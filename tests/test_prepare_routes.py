"""-m gpu: the scan preparation's routes (staged ahead, staged by the copy crew, in place: vgicp_prepare_plan.h) x the
deskew's variants, at the smallest shapes that still reach every branch."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (3_000, 70_000)
VARIANTS = ("none", "ordered-8", "ordered-4100", "swapped-8")
# copy commands the in-place route enqueues beyond the crew's: the points always; the capture times too where the crew's
# route needs no command for them (no serial walk: the prologue reads them where they are staged)
EXTRA_COPIES_IN_PLACE = {"none": 1, "ordered-8": 2, "ordered-4100": 1, "swapped-8": 1}


def _worker(stage_limit):
    env = {k: v for k, v in os.environ.items() if k != "VGICP_STAGE_LIMIT"}
    if stage_limit is not None:
        env["VGICP_STAGE_LIMIT"] = stage_limit
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prepare_routes_worker.py")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def test_every_route_prepares_what_the_stand_alone_calls_prepare():
    """One sweep of 3 000 points (one copy unit) and one of 70 000 (above the crew's helper threshold, several units), each
    without deskew, with 8 ordered states (bounds found in the prologue), 4 100 ordered states (serial walk) and 8 states
    with one swapped pair of timestamps (unordered: serial walk); prepared through scan_prepare_async and through
    sweep_stage + scan_prepare_staged_async, in a child with VGICP_STAGE_LIMIT unset (the copy crew) and in one with
    VGICP_STAGE_LIMIT=1 (in place).  Kept count, moved count, points and covariances equal, bit for bit, what vgicp_deskew
    + vgicp_preprocess (their own kernels) give on a second context.  The second child starts only if the first passed."""
    copies = {}
    for stage_limit in (None, "1"):
        d = _worker(stage_limit)
        assert d["stage_limit"] == stage_limit
        assert [(c["n"], c["variant"]) for c in d["cases"]] == [(n, v) for n in SIZES for v in VARIANTS]
        for c in d["cases"]:
            print(stage_limit, c)
            where = (stage_limit, c["n"], c["variant"])
            assert c["direct_error"] is None and c["ahead_error"] is None, where
            assert c["direct"] == c["want"] and c["ahead"] == c["want"], where
            assert c["want"][0] > 0 and (c["want"][1] > 0) == (c["variant"] != "none"), where
            assert c["direct_equal"] and c["ahead_equal"], where
            copies[where] = c["copies"]
    # the two children did take different routes: the in-place one enqueued the copy commands the crew's route saves
    for n in SIZES:
        for v in VARIANTS:
            assert copies[("1", n, v)] - copies[(None, n, v)] == EXTRA_COPIES_IN_PLACE[v], (n, v, copies)
