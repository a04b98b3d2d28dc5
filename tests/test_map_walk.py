"""The voxel map as ONE object that lives through every update in arbitrary order: seeded random walks over the whole
alphabet of map operations (tests/map_walk_reference.py: the walk, the scene, the host model), every synchronous result
and every reader of the C ABI held against the model — bit for bit, except the align's pose against the oracle's
(TIGHT_POSE_TOL) and the gate's gap, which tests/test_map_walk_cpu.py checks on the model alone.

What the walks are for is the host's bookkeeping that the entries share: voxels, tombstones and slots, map_version against
the dense copy's and every level's, what is pending (an insertion, a gate, a carve), the raw-point log's fill, the align's
memos.  The other test files pin chosen pairs of entries; a walk runs the sequences nobody thought of."""
import pytest

import map_walk_reference as mw
from conftest import TIGHT_POSE_TOL, pose_error
from test_align_batch import assert_same_bits

pytestmark = pytest.mark.gpu

COUNTER_FALLBACKS = 1


def contexts(monkeypatch, raw, **env):
    """The walked context and its twin, both created under `env` (read when a context is created, test_launch_variants.py)."""
    from eskf_lio_amd import capi
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    ctx, twin = capi.Context(0), capi.Context(0)
    for name in env:
        monkeypatch.delenv(name)
    if raw:
        ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
    return mw.Device(capi, ctx, twin, pose_error, assert_same_bits, TIGHT_POSE_TOL)


def run(oracle, monkeypatch, seed, raw, ops=None, **env):
    device = contexts(monkeypatch, raw, **env)
    with device.ctx, device.twin:
        model, events, _ = mw.run_walk(oracle, seed, raw, device, ops=ops)
        fallbacks = device.ctx.counter(COUNTER_FALLBACKS), device.twin.counter(COUNTER_FALLBACKS)
    return model, events, fallbacks


@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
@pytest.mark.parametrize("seed", mw.SEEDS)
def test_walk(oracle, monkeypatch, seed, raw):
    """48 operations, a full check of every reader at every 8th and single readers in between; with the raw-point store,
    the per-voxel lists too."""
    model, events, _ = run(oracle, monkeypatch, seed, raw)
    assert sum(e.grew for _, e in events) >= 2 and model.voxels > 0
    # every reader at each of the six full checks, the ten readers in between, and the updates that return something
    full = mw.WALK_LENGTH // mw.FULL_CHECK_EVERY * (len(mw.READERS) - (not raw))
    assert model.checks >= full + 10 + 3 + 3 + 3 + 2, model.checks


@pytest.mark.parametrize("seed", mw.SEEDS[:2])
def test_walk_reads_the_dense_copy_and_the_memos(oracle, monkeypatch, seed):
    """A context whose every table is "large" (VGICP_DENSE_SLOTS=1) and whose persistent launch has two workgroups
    (VGICP_PERSIST_GRID=2): several points per thread at 1 500 points, so the align reader goes through the dense copy —
    rebuilt when map_version says so, and only then — and the memos.  No launch gives up."""
    _, _, fallbacks = run(oracle, monkeypatch, seed, False, VGICP_DENSE_SLOTS="1", VGICP_PERSIST_GRID="2")
    assert fallbacks == (0, 0)


@pytest.mark.parametrize("seed", mw.SEEDS[2:3])
def test_walk_under_the_insertion_sort(oracle, monkeypatch, seed):
    """VGICP_INSERT_SORT: the prepared scans take the sort route too."""
    run(oracle, monkeypatch, seed, True, VGICP_INSERT_SORT="1")
