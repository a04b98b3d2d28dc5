"""The tail of the fused align and the neighbour look-ahead of the persistent rounds.

What changed under these tests: a staged unit's flag and form cross the link in ONE 8-byte load; the resident copy of
the scan (12 SoA planes + the AoS copy) leaves the fused launch write-through behind round 0's row publication; the fused
align records no marker behind its launch and starts its copy threads before the launch is set up; and the look-ahead
probes a neighbour voxel once per launch instead of once per round.  None of it may change a bit of any result, so
everything here is compared with ==, path against path, and once against the CPU oracle at the suite's tolerance.

2731 points are the smallest staged scan (96 n > 256 KB); a unit holds 2048 points, so 4095 / 4096 / 4097 end a unit, fill
two and begin a third.
"""
import numpy as np
import pytest

from conftest import POSE_TOL_M, POSE_TOL_RAD, TIGHT_POSE_TOL, pose_error

pytestmark = pytest.mark.gpu

FORCED = (1e-6, 2.0)   # thresholds no step meets: every round runs


def _context(monkeypatch, two_launch=False, margin=None):
    from eskf_lio_amd import capi
    monkeypatch.delenv("VGICP_NO_FUSED_ALIGN", raising=False)
    monkeypatch.delenv("VGICP_PREFETCH_MARGIN", raising=False)
    if two_launch:
        monkeypatch.setenv("VGICP_NO_FUSED_ALIGN", "1")
    if margin is not None:
        monkeypatch.setenv("VGICP_PREFETCH_MARGIN", margin)
    ctx = capi.Context(0)   # the switches are read here, once
    monkeypatch.delenv("VGICP_NO_FUSED_ALIGN", raising=False)
    monkeypatch.delenv("VGICP_PREFETCH_MARGIN", raising=False)
    return ctx


def _with_map(ctx, vmap):
    ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0])
    ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
    return ctx


def _same(a, b, what=""):
    assert a.iterations == b.iterations and a.converged == b.converged, what
    assert np.array_equal(a.pose, b.pose), what
    assert np.array_equal(a.normal_eq, b.normal_eq), what
    assert np.array_equal(a.corr_count, b.corr_count), what


@pytest.fixture()
def pair(monkeypatch, c1_inputs):
    """(fused context, two-launch context) over the C1 map."""
    vmap = c1_inputs[0]
    fused = _with_map(_context(monkeypatch), vmap)
    two = _with_map(_context(monkeypatch, two_launch=True), vmap)
    yield fused, two
    fused.close()
    two.close()


def _crossing_scan(n, vmap, seed):
    """A structured scan and a guess more than a voxel away from its pose: the forced rounds keep moving a tenth of the
    points into another voxel, round after round (counted in the test from the poses themselves)."""
    from eskf_lio_amd import synth
    pts, covs, _ = synth.make_structured_scan(n, vmap, seed=seed)
    return pts, covs, synth.se3_to_SE3((0.35, -0.3, 0.25, 0.02, -0.015, 0.02))


def _voxel_keys(T, pts, h):
    return np.floor((pts @ T[:3, :3].T + T[:3, 3]) / h).astype(np.int64)


# ---- the unit's form arrives with its flag ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2731, 4095, 4096, 4097])
def test_form_and_flag_in_one_load(pair, c1_inputs, c1_oracle_map, n):
    """One asymmetric covariance in the first unit, in the last unit, nowhere: compact and full units in one launch.  The
    fused align, the two-launch path and the launch-per-round loop return the same bits; the oracle agrees."""
    from eskf_lio_amd import capi, synth
    fused, two = pair
    vmap = c1_inputs[0]
    g = synth.default_guess()
    for where in (0, n - 1, None):
        pts, covs = synth.make_uniform_scan(n, vmap, seed=4000 + n)
        covs = covs.copy()
        if where is not None:
            covs[where, 1] += 1e-9            # c10 != c01: that unit crosses the link whole
        fused.frame_stats(reset=True)
        a = fused.align(pts.copy(), covs.copy(), g, 8, *FORCED)
        assert fused.frame_stats(reset=True).kernel_launches == 1, (n, where)   # the fused path was taken
        b = two.align(pts.copy(), covs.copy(), g, 8, *FORCED)
        c = two.align(pts.copy(), covs.copy(), g, 8, *FORCED, flags=capi.FLAG_NO_PERSISTENT)
        _same(a, b, (n, where, "two launches"))
        _same(a, c, (n, where, "loop"))
        for ctx in (fused, two):
            dp, dc = ctx.scan_download()
            assert np.array_equal(dp, pts) and np.array_equal(dc, covs), (n, where)
        ref = c1_oracle_map.align(pts, covs, g, 8, *FORCED)
        assert a.iterations == ref.iterations and a.converged == ref.converged
        assert np.array_equal(a.corr_count, ref.corr_count)
        dt, dr = pose_error(a.pose, ref.pose)
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and dt <= TIGHT_POSE_TOL and dr <= TIGHT_POSE_TOL, (n, where, dt, dr)


# ---- the resident copy the fused launch leaves behind -------------------------------------------------------------------
def test_resident_copy_after_a_fused_align(monkeypatch, c1_inputs):
    """n = 4097 (three units, an odd count): the download returns the caller's arrays bit for bit, and what reads the
    resident scan next — a resident align (SoA planes), a map insertion (AoS copy) — does what it does after
    vgicp_scan_upload."""
    from eskf_lio_amd import synth
    vmap = c1_inputs[0]
    g = synth.default_guess()
    pts, covs = synth.make_uniform_scan(4097, vmap, seed=91)
    covs = covs.copy()
    covs[4096, 5] += 1e-9                     # the last unit whole, the others compact
    fused = _with_map(_context(monkeypatch), vmap)
    plain = _with_map(_context(monkeypatch), vmap)
    try:
        fused.frame_stats(reset=True)
        a = fused.align(pts.copy(), covs.copy(), g, 6, *FORCED)
        assert fused.frame_stats(reset=True).kernel_launches == 1
        dp, dc = fused.scan_download()
        assert np.array_equal(dp, pts) and np.array_equal(dc, covs)
        plain.scan_upload(pts.copy(), covs.copy())
        _same(a, plain.align_resident(g, 6, *FORCED), "upload + resident align")
        _same(fused.align_resident(g, 9, *FORCED), plain.align_resident(g, 9, *FORCED), "resident align")
        for ctx in (fused, plain):
            ctx.map_insert_resident_async(a.pose, 20)
        assert fused.map_size() == plain.map_size() and fused.map_size()[0] > vmap.keys.shape[0]
        _same(fused.align_resident(g, 6, *FORCED), plain.align_resident(g, 6, *FORCED), "after the insertion")
    finally:
        fused.close()
        plain.close()


# ---- the look-ahead: one probe per neighbour and launch -----------------------------------------------------------------
@pytest.mark.parametrize("n", [449, 4097])
def test_look_ahead_changes_no_result_and_keeps_no_memo(monkeypatch, c1_inputs, n):
    """n = 449: two workgroups of the plain persistent launch; n = 4097: the fused one.  Margins 0 (no look-ahead), the
    default and 0.2 (two points in five look ahead) return the same bits; so does a second align on the same context
    after the map lost and changed voxels, against a context that never saw the old map."""
    from eskf_lio_amd import synth
    vmap = c1_inputs[0]
    h = vmap.voxel_size
    pts, covs, g = _crossing_scan(n, vmap, seed=11)
    ctxs = [_with_map(_context(monkeypatch, margin=m), vmap) for m in ("0", None, "0.2")]
    fresh = []
    try:
        first = [ctx.align(pts.copy(), covs.copy(), g, 10, *FORCED) for ctx in ctxs]
        assert first[0].iterations == 10
        _same(first[0], first[1], "margin 0 / default")
        _same(first[0], first[2], "margin 0 / 0.2")
        # the scan does what it was built for: points change voxel in each of the first six rounds
        prev = g
        for k in range(1, 7):
            pose = ctxs[0].align(pts.copy(), covs.copy(), g, k, *FORCED).pose
            crossed = int((_voxel_keys(prev, pts, h) != _voxel_keys(pose, pts, h)).any(axis=1).sum())
            assert crossed >= n // 50, (k, crossed)
            prev = pose
        # the map changes under the contexts: every third voxel the scan touches at the final pose goes, every third
        # moves its mean
        touched = np.unique(_voxel_keys(first[0].pose, pts, h), axis=0).astype(np.int32)
        index = {tuple(k): i for i, k in enumerate(vmap.keys.tolist())}
        rows = np.array([index[tuple(k)] for k in touched.tolist() if tuple(k) in index])
        gone, moved = rows[0::3], rows[1::3]
        assert len(gone) > n // 20 and len(moved) > n // 20

        def change(ctx):
            ctx.map_erase(vmap.keys[gone])
            ctx.map_upsert(vmap.keys[moved], vmap.means[moved] + 0.01, vmap.covs[moved])

        for m, ctx in zip(("0", None, "0.2"), ctxs):
            change(ctx)
            other = _with_map(_context(monkeypatch, margin=m), vmap)
            fresh.append(other)
            change(other)
        second = [ctx.align(pts.copy(), covs.copy(), g, 10, *FORCED) for ctx in ctxs]
        again = [ctx.align(pts.copy(), covs.copy(), g, 10, *FORCED) for ctx in fresh]
        assert not np.array_equal(second[0].corr_count, first[0].corr_count)   # the change was felt
        for s, f in zip(second, again):
            _same(s, f, "same context / fresh context")
        _same(second[0], second[1], "margin 0 / default, changed map")
        _same(second[0], second[2], "margin 0 / 0.2, changed map")
    finally:
        for ctx in ctxs + fresh:
            ctx.close()


# ---- the host path: no marker behind the fused launch -------------------------------------------------------------------
def test_staging_memory_across_fused_aligns_and_uploads(pair, c1_inputs):
    """Fused aligns of growing size back to back (the staging memory is replaced twice while the context believes the
    last launch synchronised), then vgicp_scan_upload (which leaves its marker) + a resident align, then a fused align
    again: every result is the two-launch path's, no upload counted slow, no persistent fallback."""
    from eskf_lio_amd import capi, synth
    fused, two = pair
    vmap = c1_inputs[0]
    g = synth.default_guess()
    before = [(c.counter(capi.COUNTER_UPLOAD_SLOW), c.counter(1)) for c in (fused, two)]
    for n in (3_001, 30_001, 60_001, 100_001, 2_731):
        pts, covs = synth.make_uniform_scan(n, vmap, seed=600 + n)
        fused.frame_stats(reset=True)
        a = fused.align(pts.copy(), covs.copy(), g, 5, *FORCED)
        assert fused.frame_stats(reset=True).kernel_launches == 1, n
        _same(a, two.align(pts.copy(), covs.copy(), g, 5, *FORCED), n)
        dp, dc = fused.scan_download()
        assert np.array_equal(dp, pts) and np.array_equal(dc, covs), n
    pts, covs = synth.make_uniform_scan(120_001, vmap, seed=7)       # larger than any before: the stage grows under a marker
    for ctx in (fused, two):
        ctx.scan_upload(pts.copy(), covs.copy())
    _same(fused.align_resident(g, 5, *FORCED), two.align_resident(g, 5, *FORCED), "upload + resident")
    pts, covs = synth.make_uniform_scan(50_001, vmap, seed=8)
    fused.frame_stats(reset=True)
    a = fused.align(pts.copy(), covs.copy(), g, 5, *FORCED)
    assert fused.frame_stats(reset=True).kernel_launches == 1
    _same(a, two.align(pts.copy(), covs.copy(), g, 5, *FORCED), "fused again")
    dp, dc = fused.scan_download()
    assert np.array_equal(dp, pts) and np.array_equal(dc, covs)
    assert [(c.counter(capi.COUNTER_UPLOAD_SLOW), c.counter(1)) for c in (fused, two)] == before
