"""vgicp_scan_fetch_begin / _end on the call paths the bit-exact fetch tests in test_gpu_parity.py do not take: refused
scans, calls made between the two halves, a multi-device context, and a staged sweep's ticket used from two threads.

"Reference bits" are what a FRESH context's vgicp_scan_prepare + vgicp_scan_download make of the same input (the
two-step path, no fetch kernel involved); the oracle's transform -> deskew -> preprocess chain anchors them.  A refused
scan (a point beyond the search grid) must be reported within REFUSAL_SECONDS of wall time, and whatever
vgicp_scan_fetch_end delivers must be the scan resident at that moment, bit for bit."""
import threading
import time

import numpy as np
import pytest

from eskf_lio_amd import capi, synth
from test_gpu_parity import _assert_fetch_sums

pytestmark = pytest.mark.gpu

REFUSAL_SECONDS = 1.0
VOXEL = 0.3
KNN = 30
# one far point (a corrupt return) at the first, a middle and the last index; +1e9 in x, then -1e9 in z
FAR_POINTS = [(where, axis, value) for axis, value in ((0, 1e9), (2, -1e9)) for where in ("first", "middle", "last")]
# how the sweep reaches the preparation; "staged" comes without capture times, "cloud2" with them
KINDS = ("async", "async_deskew", "staged", "cloud2")


def _states():
    return synth.make_imu_states(48, seed=5)


def _extrinsic():
    return synth.se3_to_SE3([0.01, -0.02, 0.03, 0.002, -0.001, 0.003])


def _sweep(n, seed):
    st = _states()
    pts = synth.make_lidar_scan(n, seed=seed)
    tt = synth.make_point_times(n, st[1, 0] + 1e-4, st[-3, 0] + 0.4 / 400.0, seed=seed)
    return pts, tt


def _records(pts, tt):
    """A PointCloud2 payload: float32 x y z at bytes 0 / 4 / 8, a float64 capture time at 16, 24 bytes a record."""
    n = len(pts)
    rec = np.zeros((n, 24), dtype=np.uint8)
    for c in range(3):
        rec[:, 4 * c:4 * c + 4] = pts[:, c].astype("<f4").view(np.uint8).reshape(n, 4)
    rec[:, 16:24] = tt.astype("<f8").view(np.uint8).reshape(n, 8)
    return rec


def _deskews(kind):
    return kind in ("async_deskew", "cloud2")


def _prepare(ctx, kind, pts, tt):
    """One enqueued preparation of the sweep through the entry point `kind` names."""
    st = _states() if _deskews(kind) else None
    if kind.startswith("async"):
        ctx.scan_prepare_async(pts, tt if st is not None else None, st, _extrinsic(), VOXEL, KNN)
    elif kind == "staged":
        ctx.scan_prepare_staged_async(ctx.sweep_stage(pts), st, _extrinsic(), VOXEL, KNN)
    else:
        ticket = ctx.sweep_stage_cloud2(_records(pts, tt), len(pts), 24, 0, 4, 8, 16)
        ctx.scan_prepare_staged_async(ticket, st, _extrinsic(), VOXEL, KNN)


def _reference(oracle, kind, pts, tt):
    """(points, covs, voxels after one insertion into an empty map) from a fresh context's two-step path, checked
    against the oracle chain."""
    if kind == "cloud2":
        pts = pts.astype(np.float32).astype(np.float64)   # what the device widens the wire floats to
    st = _states() if _deskews(kind) else None
    with capi.Context(0) as ref:
        ref.map_reset(VOXEL, 0)
        kept, _ = ref.scan_prepare(pts, tt if st is not None else None, st, _extrinsic(), VOXEL, KNN)
        rp, rc = ref.scan_download()
        ref.map_insert_resident_async(np.eye(4), 20)
        voxels = ref.map_size()[0]
    moved, _ = oracle.transform(pts, np.tile(np.eye(3).reshape(9), (len(pts), 1)), _extrinsic())
    if st is not None:
        moved, done = oracle.deskew(moved, tt, st)
        assert done > 0
    op, oc, _ = oracle.preprocess(moved, VOXEL, KNN)
    assert kept == len(rp) == len(op) and np.array_equal(rp, op) and np.array_equal(rc, oc), kind
    return rp, rc, voxels


def _fetch(ctx, capacity=None):
    kept = ctx.scan_fetch_begin()
    return ctx.scan_fetch_end(kept if capacity is None else capacity)


def _refused_fetch(ctx):
    """begin + end of a refused scan -> (status, wall seconds of the two calls)."""
    t0 = time.perf_counter()
    with pytest.raises(capi.VgicpError) as e:
        kept = ctx.scan_fetch_begin()
        ctx.scan_fetch_end(kept)
    return e.value.code, time.perf_counter() - t0


def _far_index(where, n):
    return {"first": 0, "middle": n // 2, "last": n - 1}[where]


@pytest.mark.parametrize("n", (2_731, 30_001))
@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_scan_fails_the_fetch_at_once_and_the_context_recovers(oracle, kind, n):
    """A scan with one point beyond the search grid, prepared through every enqueued entry point, with the far point
    first, in the middle and last: the fetch reports VGICP_ERR_BAD_ARGUMENT within REFUSAL_SECONDS (it must not wait
    for pieces a refused scan never writes), no checksums are offered, and the same context then prepares, fetches
    and inserts a good sweep exactly as a fresh context does.  Both sizes keep enough points to span several 64 KB
    pieces."""
    pts, tt = _sweep(n, seed=40 + n % 97)
    rp, rc, voxels = _reference(oracle, kind, pts, tt)
    with capi.Context(0) as ctx:
        ctx.map_reset(VOXEL, 0)
        _prepare(ctx, kind, pts, tt)             # warm: every kernel of the path has run once in this process
        fp, fc = _fetch(ctx)
        assert np.array_equal(fp, rp) and np.array_equal(fc, rc)
        for where, axis, value in FAR_POINTS:
            what = (kind, n, where, axis, value)
            bad = pts.copy()
            bad[_far_index(where, n), axis] = value
            _prepare(ctx, kind, bad, tt)
            code, seconds = _refused_fetch(ctx)
            assert code == capi.ERR_BAD_ARGUMENT, what
            assert seconds <= REFUSAL_SECONDS, (what, seconds)
            with pytest.raises(capi.VgicpError) as e:
                ctx.scan_fetch_sums()
            assert e.value.code == capi.ERR_NOT_READY, what
            ctx.map_reset(VOXEL, 0)
            _prepare(ctx, kind, pts, tt)
            fp, fc = _fetch(ctx)
            assert np.array_equal(fp, rp) and np.array_equal(fc, rc), what
            _assert_fetch_sums(ctx.scan_fetch_sums(), fp, fc, what)
            ctx.map_insert_resident_async(np.eye(4), 20)
            assert ctx.map_size()[0] == voxels, what


def test_the_drop_in_preprocessor_reports_a_refused_sweep_at_once(oracle):
    """CloudPreprocessor::process with the eager host copy (the drop-in's fetch pair): a sweep with one far point throws
    within REFUSAL_SECONDS, and the next process() on the same object equals the oracle chain bit for bit."""
    from eskf_lio_amd import host
    n = 20_000
    st = synth.make_imu_states(48, seed=31)
    T_il = synth.se3_to_SE3(np.array([0.05, -0.02, 0.1, 0.01, -0.02, 0.03]))
    pre = host.CloudPreprocessor(VOXEL, T_il, host_copy="eager")

    def expected(pts, t):
        moved, _ = oracle.transform(pts, np.tile(np.eye(3).reshape(9), (n, 1)), T_il)
        desk, done = oracle.deskew(moved, t, st)
        assert done > 0
        return oracle.preprocess(desk, VOXEL, KNN)[:2]

    for seed in (31, 32):
        pts = synth.make_lidar_scan(n, seed=seed)
        t = synth.make_point_times(n, st[1, 0] + 1e-4, st[-3, 0] + 1e-3, seed=seed)
        if seed == 31:                             # warm, and the object works before the refusal
            gp, gc = pre.process(st, pts, t)
            rp, rc = expected(pts, t)
            assert np.array_equal(gp, rp) and np.array_equal(gc, rc)
            bad = pts.copy()
            bad[n // 2, 0] = 1e9
            t0 = time.perf_counter()
            with pytest.raises(RuntimeError):
                pre.process(st, bad, t.copy())
            seconds = time.perf_counter() - t0
            assert seconds <= REFUSAL_SECONDS, seconds
        else:
            gp, gc = pre.process(st, pts, t)
            rp, rc = expected(pts, t)
            assert np.array_equal(gp, rp) and np.array_equal(gc, rc)


def _delivered(ctx, got, want, stale=None, sums_required=False):
    """What fetch_end delivered is `want` bit for bit (never `stale`); the checksums match it or are not offered."""
    gp, gc = got
    assert len(gp) == len(want[0]) and np.array_equal(gp, want[0]) and np.array_equal(gc, want[1])
    if stale is not None:
        assert not np.array_equal(gp, stale[0])
    try:
        sums = ctx.scan_fetch_sums()
    except capi.VgicpError as e:
        assert e.code == capi.ERR_NOT_READY and not sums_required
        return
    _assert_fetch_sums(sums, gp, gc, "delivered")


@pytest.mark.parametrize("devices", (0, [0, 0]), ids=("one_device", "multi_device"))
def test_calls_between_fetch_begin_and_end(oracle, devices):
    """Every order of calls around the fetch pair delivers the scan that is resident when vgicp_scan_fetch_end is called.
    A and B keep the same number of points with different bytes (B is A reversed: the same voxels, other first
    points), so a stale copy of A cannot hide behind a size check.  On a multi-device context the pair is the two-step
    path, and the answers are the same."""
    multi = isinstance(devices, list)
    A = synth.make_lidar_scan(9_000, seed=71)
    B = np.ascontiguousarray(A[::-1])
    ext = _extrinsic()
    refA = _reference(oracle, "async", A, None)
    refB = _reference(oracle, "async", B, None)
    kA = len(refA[0])
    assert kA == len(refB[0]) and not np.array_equal(refA[0], refB[0])
    guess = synth.se3_to_SE3([0.05, -0.03, 0.02, 0.002, -0.001, 0.003])

    def prep(ctx, pts):
        ctx.scan_prepare_async(pts, None, None, ext, VOXEL, KNN)

    with capi.Context(devices) as ctx, capi.Context(devices) as first:
        for c in (ctx, first):
            c.map_reset(VOXEL, 0)
            c.map_insert_scan(refA[0], refA[1], np.eye(4), 20)
        valid = not multi   # the fetch kernel's checksums exist on a single-device context only

        # a new preparation between begin and end: the new scan, not the copy begun for the old one
        prep(ctx, A)
        assert ctx.scan_fetch_begin() == kA
        prep(ctx, B)
        _delivered(ctx, ctx.scan_fetch_end(kA), refB, stale=refA)
        # ... and a second begin for it
        prep(ctx, A)
        ctx.scan_fetch_begin()
        prep(ctx, B)
        assert ctx.scan_fetch_begin() == kA
        _delivered(ctx, ctx.scan_fetch_end(kA), refB, stale=refA, sums_required=valid)

        # an align between begin and end reads the scan and leaves it resident: A, and the align of a context that fetched first
        prep(ctx, A)
        assert ctx.scan_fetch_begin() == kA
        got = ctx.align_resident(guess, 10, 1e-6, 0.9999)
        _delivered(ctx, ctx.scan_fetch_end(kA), refA, sums_required=valid)
        prep(first, A)
        _delivered(first, _fetch(first), refA, sums_required=valid)
        want = first.align_resident(guess, 10, 1e-6, 0.9999)
        assert got.iterations == want.iterations and np.array_equal(got.corr_count, want.corr_count)
        if multi:   # the sub-contexts' rows are added in a fixed order, or on the host when they cannot meet in the kernel
            assert float(np.abs(got.pose - want.pose).max()) <= 1e-11
        else:
            assert np.array_equal(got.pose, want.pose) and np.array_equal(got.normal_eq, want.normal_eq)

        # an upload between begin and end replaces the scan: the uploaded one (as many points as A)
        prep(ctx, A)
        assert ctx.scan_fetch_begin() == kA
        ctx.scan_upload(refB[0], refB[1])
        _delivered(ctx, ctx.scan_fetch_end(kA), refB, stale=refA)

        # begin twice
        prep(ctx, A)
        ctx.scan_fetch_begin()
        assert ctx.scan_fetch_begin() == kA
        _delivered(ctx, ctx.scan_fetch_end(kA), refA, sums_required=valid)

        # end without begin: the two-step answer
        prep(ctx, B)
        _delivered(ctx, ctx.scan_fetch_end(kA), refB, stale=refA)

        # a capacity one short: refused, no checksums, and the next fetches are right
        prep(ctx, A)
        assert ctx.scan_fetch_begin() == kA
        with pytest.raises(capi.VgicpError) as e:
            ctx.scan_fetch_end(kA - 1)
        assert e.value.code == capi.ERR_BAD_ARGUMENT
        with pytest.raises(capi.VgicpError) as e:
            ctx.scan_fetch_sums()
        assert e.value.code == capi.ERR_NOT_READY
        _delivered(ctx, _fetch(ctx), refA)
        prep(ctx, B)
        _delivered(ctx, _fetch(ctx), refB, stale=refA, sums_required=valid)


def test_a_staged_ticket_is_used_once_under_two_threads(oracle):
    """vgicp_scan_prepare_staged_async on the owner thread and vgicp_sweep_unstage of the same ticket on another, started
    together (ctypes releases the GIL inside both calls), then a vgicp_sweep_stage of another sweep of the same size:
    exactly one of the two uses of the ticket succeeds, and when the preparation wins, its scan is the first sweep's,
    bit for bit — the stage that follows never refills the slot it is reading."""
    n = 20_000
    first = synth.make_lidar_scan(n, seed=81)
    other = synth.make_lidar_scan(n, seed=82)
    with capi.Context(0) as ref:
        ref.scan_prepare(first, None, None, None, VOXEL, KNN)
        rp, rc = ref.scan_download()
    op, oc, _ = oracle.preprocess(first, VOXEL, KNN)
    assert np.array_equal(rp, op) and np.array_equal(rc, oc)
    barrier = threading.Barrier(2, timeout=60)
    outcome = {}

    def dropper(ticket):
        barrier.wait()
        try:
            ctx.sweep_unstage(ticket)
            outcome["unstaged"] = True
        except capi.VgicpError as e:
            outcome["unstaged"] = e.code
        outcome["second"] = ctx.sweep_stage(other)

    prepared = unstaged = 0
    with capi.Context(0) as ctx:
        ctx.map_reset(VOXEL, 0)
        for round_ in range(200):
            outcome.clear()
            ticket = ctx.sweep_stage(first)
            th = threading.Thread(target=dropper, args=(ticket,))
            th.start()
            barrier.wait()
            try:
                ctx.scan_prepare_staged_async(ticket, None, None, VOXEL, KNN)
                won = True
            except capi.VgicpError as e:
                assert e.code == capi.ERR_BAD_ARGUMENT, round_
                won = False
            th.join(timeout=60)
            assert not th.is_alive() and "second" in outcome, (round_, outcome)
            assert won != (outcome["unstaged"] is True), (round_, won, outcome)
            if won:
                assert outcome["unstaged"] == capi.ERR_BAD_ARGUMENT, (round_, outcome)
                fp, fc = _fetch(ctx)
                assert np.array_equal(fp, rp) and np.array_equal(fc, rc), round_
                prepared += 1
            else:
                unstaged += 1
            ctx.sweep_unstage(outcome["second"])   # the other sweep is dropped: its slot is free again
    assert prepared + unstaged == 200
