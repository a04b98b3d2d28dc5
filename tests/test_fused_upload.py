"""The fused align: vgicp_align of a staged scan in ONE persistent launch whose workgroups read their points out of the
page-locked staging memory themselves, against the two-launch path (pack_arena_kernel, then the persistent launch) that
VGICP_NO_FUSED_ALIGN keeps.  Both must return the same bits and leave the same resident scan behind."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _context(monkeypatch, two_launch: bool, threads: str | None = None):
    from eskf_lio_amd import capi
    if two_launch:
        monkeypatch.setenv("VGICP_NO_FUSED_ALIGN", "1")
    else:
        monkeypatch.delenv("VGICP_NO_FUSED_ALIGN", raising=False)
    if threads is not None:
        monkeypatch.setenv("VGICP_UPLOAD_THREADS", threads)
    ctx = capi.Context(0)   # the switches are read here, once
    monkeypatch.delenv("VGICP_NO_FUSED_ALIGN", raising=False)
    monkeypatch.delenv("VGICP_UPLOAD_THREADS", raising=False)
    return ctx


def _with_map(ctx, vmap):
    ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0])
    ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
    return ctx


def _same(a, b):
    assert a.iterations == b.iterations and a.converged == b.converged
    assert np.array_equal(a.pose, b.pose)
    assert np.array_equal(a.normal_eq, b.normal_eq)
    assert np.array_equal(a.corr_count, b.corr_count)


@pytest.fixture(scope="module")
def fused_map():
    from eskf_lio_amd import synth
    return synth.make_map(200_000)


@pytest.fixture()
def pair(monkeypatch, fused_map):
    """(fused context, two-launch context), both holding the same map."""
    fused = _with_map(_context(monkeypatch, False), fused_map)
    two = _with_map(_context(monkeypatch, True), fused_map)
    yield fused, two
    fused.close()
    two.close()


def _align_both(fused, two, pts, covs, iters=8):
    from eskf_lio_amd import synth
    g = synth.default_guess()
    fused.frame_stats(reset=True)
    a = fused.align(pts.copy(), covs.copy(), g, iters, 1e-6, 2.0)
    fused_launches = fused.frame_stats(reset=True).kernel_launches
    b = two.align(pts.copy(), covs.copy(), g, iters, 1e-6, 2.0)
    _same(a, b)
    for ctx in (fused, two):
        dp, dc = ctx.scan_download()
        assert np.array_equal(dp, pts) and np.array_equal(dc, covs)
    return a, b, fused_launches


@pytest.mark.gpu
def test_fused_align_matches_two_launches_at_unit_and_grid_edges(pair, fused_map):
    from eskf_lio_amd import synth
    fused, two = pair
    _, cu, _ = fused.device_info()
    grid = min(cu, 256)
    sizes = [2_047, 2_048, 2_049, 2_731, 4_095, 4_096, 4_097, 6_145, 30_001, 100_000, grid * 448, grid * 448 + 1]
    for n in sizes:
        pts, covs = synth.make_uniform_scan(n, fused_map, seed=1000 + n)
        a, b, launches = _align_both(fused, two, pts, covs)
        assert a.launches == 1 and b.launches == 1
        staged = n * 96 > 256 * 1024
        if staged and n <= grid * 448:
            assert launches == 1, n            # the upload rode inside the registration launch
        else:
            assert launches >= 2, n            # the pack (or the runtime's copy) in front, as before
    assert fused.counter(1) == 0 and two.counter(1) == 0
    assert fused.counter(6) == 0 and two.counter(6) == 0


@pytest.mark.gpu
def test_fused_align_with_one_asymmetric_covariance(pair, fused_map):
    from eskf_lio_amd import synth
    fused, two = pair
    for n, where in ((30_001, 17_000), (4_097, 4_096), (4_097, 0)):
        pts, covs = synth.make_uniform_scan(n, fused_map, seed=77 + where)
        covs = covs.copy()
        covs[where, 1] += 1e-9            # c01 != c10: that unit crosses the link whole
        _, _, launches = _align_both(fused, two, pts, covs)
        assert launches == 1
        # the resident scan's verdict: the next resident align reads all twelve planes on both paths
        g = synth.default_guess()
        _same(fused.align_resident(g, 6, 1e-6, 2.0), two.align_resident(g, 6, 1e-6, 2.0))


@pytest.mark.gpu
@pytest.mark.parametrize("threads", ["1", "2", "4"])
def test_fused_align_with_each_number_of_copy_threads(monkeypatch, fused_map, threads):
    from eskf_lio_amd import synth
    fused = _with_map(_context(monkeypatch, False, threads), fused_map)
    two = _with_map(_context(monkeypatch, True, threads), fused_map)
    try:
        for n in (40_000, 100_000):
            pts, covs = synth.make_uniform_scan(n, fused_map, seed=5 + n)
            _, _, launches = _align_both(fused, two, pts, covs, iters=6)
            assert launches == 1
    finally:
        fused.close()
        two.close()


@pytest.mark.gpu
def test_resident_align_and_map_insertion_after_a_fused_align(pair, fused_map):
    from eskf_lio_amd import synth
    fused, two = pair
    pts, covs = synth.make_uniform_scan(60_001, fused_map, seed=31)
    a, _, launches = _align_both(fused, two, pts, covs)
    assert launches == 1
    g = synth.default_guess()
    _same(fused.align_resident(g, 10, 1e-6, 2.0), two.align_resident(g, 10, 1e-6, 2.0))
    created = [ctx.map_insert_scan(pts, covs, a.pose, 20) for ctx in (fused, two)]
    assert created[0] == created[1] and fused.map_size() == two.map_size()
    # the next fused align registers against the grown map exactly as the two-launch path does
    pts2, covs2 = synth.make_uniform_scan(50_000, fused_map, seed=32)
    _, _, launches = _align_both(fused, two, pts2, covs2)
    assert launches == 1


@pytest.mark.gpu
def test_fused_align_whose_copy_threads_are_held_up():
    """The copy thread sleeps 150 ms and the workgroups wait for one poll only: the fused launch gives up, the host
    packs the staged scan and runs the align again.  Same bits as the two-launch path, one slow upload, no persistent
    fallback (a slow host is not a sign of a busy device)."""
    code = textwrap.dedent("""
        import os, sys
        import numpy as np
        sys.path.insert(0, %r)
        from eskf_lio_amd import capi, synth
        vmap = synth.make_map(50_000)
        g = synth.default_guess()
        results = []
        for two_launch in (False, True):
            if two_launch:
                os.environ["VGICP_NO_FUSED_ALIGN"] = "1"
                for k in ("VGICP_PACK_SPIN_LIMIT", "VGICP_DEBUG_UPLOAD_DELAY_US"):
                    os.environ.pop(k)
            with capi.Context(0) as ctx:
                ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0]); ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
                for n in (9_000, 30_001):
                    pts, covs = synth.make_uniform_scan(n, vmap, seed=n)
                    r = ctx.align(pts.copy(), covs.copy(), g, 6, 1e-6, 2.0)
                    dp, dc = ctx.scan_download()
                    assert np.array_equal(dp, pts) and np.array_equal(dc, covs)
                    results.append(r)
                if not two_launch:
                    assert ctx.counter(capi.COUNTER_UPLOAD_SLOW) == 2, ctx.counter(capi.COUNTER_UPLOAD_SLOW)
                    assert ctx.counter(1) == 0, ctx.counter(1)
                    # after the slow uploads the single launch is still in use (no cooldown)
                    assert all(r.launches == 1 for r in results)
        for a, b in zip(results[:2], results[2:]):
            assert np.array_equal(a.pose, b.pose) and np.array_equal(a.normal_eq, b.normal_eq)
            assert np.array_equal(a.corr_count, b.corr_count)
        print("ok")
    """ % ROOT)
    env = dict(os.environ, VGICP_PACK_SPIN_LIMIT="1", VGICP_DEBUG_UPLOAD_DELAY_US="150000", VGICP_UPLOAD_THREADS="1")
    env.pop("VGICP_NO_FUSED_ALIGN", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.gpu
def test_fused_align_reports_the_registration_device_time(pair, fused_map):
    """stats.device_seconds of a fused align: from the last unit to the end of the launch, not the upload."""
    from eskf_lio_amd import synth
    fused, two = pair
    pts, covs = synth.make_uniform_scan(100_000, fused_map, seed=3)
    a = [fused.align(pts.copy(), covs.copy(), synth.default_guess(), 20, 1e-6, 2.0) for _ in range(5)][-1]
    b = [two.align(pts.copy(), covs.copy(), synth.default_guess(), 20, 1e-6, 2.0) for _ in range(5)][-1]
    assert 0.0 < a.device_seconds < 2.0 * b.device_seconds
