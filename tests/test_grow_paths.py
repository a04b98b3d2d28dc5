"""-m gpu: every buffer of a context that grows after creation grows here, in one process, three times over: voxel table
(rehash, the raw-point log following it), raw-point log, resident scan, staging area, cell table, page-locked sweep
staging, a slot of the sweeps staged ahead, the scan fetch's staging, the dense copy, the iteration log.  A block that
is replaced while something still reads or writes the old one shows as a result that differs from run to run."""
import numpy as np
import pytest

from conftest import TIGHT_POSE_TOL
from test_gpu_parity import assert_align_parity

pytestmark = pytest.mark.gpu
VOXEL = 0.3
SIZES = (3_000, 70_000)   # the two sizes of tests/test_prepare_routes.py: one copy unit; several, above the crew's helper threshold
POINTS_PER_VOXEL = 20
GUESS_XI = [0.004, -0.003, 0.002, 0.001, -0.002, 0.0015]


def _same(a, b):
    """bit for bit: arrays by their bytes (a NaN equals itself, -0.0 is not 0.0), everything else by =="""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _align_record(r):
    return [r.pose, r.iterations, r.converged, r.corr_count, r.JTJ, r.JTr]


def _walk(monkeypatch, sweeps, guess, oracle=None):
    """One context from creation to destruction -> everything it returned, in call order."""
    from eskf_lio_amd import capi
    out = []
    monkeypatch.setenv("VGICP_DENSE_SLOTS", "1")   # read at creation: every table gets a dense copy, sized with the table
    with capi.Context(0) as ctx:
        monkeypatch.delenv("VGICP_DENSE_SLOTS")
        ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
        ctx.map_reset(VOXEL, 0)                    # no hint: the smallest table (1024 slots) and the smallest raw-point log
        assert ctx.map_size() == (0, 1024)
        for n, raw in zip(SIZES, sweeps):
            # scan, staging area, cell table and the crew's page-locked sweep staging are sized by the sweep
            ctx.scan_prepare_async(raw, None, None, None, VOXEL, 30)
            kept = ctx.scan_fetch_begin()          # ... and the fetch's staging by what the preparation kept
            pts, covs = ctx.scan_fetch_end(kept)
            assert len(pts) == kept and 512 < kept <= n
            out += [kept, pts, covs, ctx.scan_fetch_sums(), ctx.scan_info()]
            # more new voxels than half the table's slots: the table is made anew, and from the second sweep on its
            # records are rehashed and the raw points move with them; the raw-point log is compacted and grows
            slots_before = ctx.map_size()[1]
            new = ctx.map_insert_resident(np.eye(4), POINTS_PER_VOXEL)
            voxels, slots = ctx.map_size()
            assert new > 512 and slots > slots_before and 2 * voxels <= slots
            out += [new, voxels, slots, ctx.map_points_size()]
            if n == SIZES[0]:
                got = ctx.align_resident(guess, 20, 1e-6, 2.0)
                out += _align_record(got)
                if oracle is not None:             # the same align on the CPU: the map as exported, the scan as fetched
                    keys, means, mcovs, _ = ctx.map_export()
                    omap = oracle.OracleMap(VOXEL, 1)
                    omap.insert(means, mcovs)
                    assert len(omap) == len(keys)
                    assert_align_parity(got, omap.align(pts, covs, guess, 20, 1e-6, 2.0), tight=TIGHT_POSE_TOL)
        # the large sweep again, staged ahead: a slot of the staged sweeps grows, the preparation reads it from there
        ctx.scan_prepare_staged_async(ctx.sweep_stage(sweeps[1]), None, None, VOXEL, 30)
        kept = ctx.scan_fetch_begin()
        out += [kept, *ctx.scan_fetch_end(kept), ctx.scan_fetch_sums()]
        assert _same(out[-3:-1], [pts, covs])      # the same sweep prepared by the other route: the same scan
        a = ctx.align_resident(guess, 20, 1e-6, 2.0)
        b = ctx.align_resident(guess, 200, 1e-6, 2.0)   # past the log's first 128 rows: the log is made anew
        assert a.iterations == 20 and b.iterations == 200
        out += _align_record(a) + _align_record(b)
        out += list(ctx.map_export())
        keys, points = ctx.map_points_export()     # the voxels come in no promised order: sorted by voxel, then by point
        order = np.lexsort((points[:, 2], points[:, 1], points[:, 0], keys[:, 2], keys[:, 1], keys[:, 0]))
        out += [keys[order], points[order]]
    return out


def test_every_grow_path_three_times_in_one_process(monkeypatch, oracle):
    """Per context: VGICP_DENSE_SLOTS=1, raw points on, a table of 1024 slots; a sweep of 3 000 points prepared, fetched and
    inserted (more than 512 new voxels), then one of 70 000; the large one again through vgicp_sweep_stage +
    vgicp_scan_prepare_staged_async; aligns of 20 and of 200 forced rounds; the map and its raw points exported; the
    context destroyed.  Three contexts in a row: every pose, count, checksum, fetched scan and exported record of the
    second and third equals the first's bit for bit.  The first run's align at the 3 000-point size is also held against
    the oracle's, with the bounds of test_gpu_parity.py (identical counts, 1e-9 m / rad)."""
    from eskf_lio_amd import synth
    sweeps = [synth.make_lidar_scan(n, seed=41, extent=30.0) for n in SIZES]
    guess = synth.se3_to_SE3(GUESS_XI)
    first = _walk(monkeypatch, sweeps, guess, oracle)
    for run in (2, 3):
        again = _walk(monkeypatch, sweeps, guess)
        assert len(again) == len(first)
        differ = [i for i, (x, y) in enumerate(zip(first, again)) if not _same(x, y)]
        assert not differ, (run, differ)
