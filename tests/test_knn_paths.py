"""The neighbour search of the scan preparation on scans built to take each of its paths (tests/knn_paths_reference.py).

knn_search_kernel reaches the exact k nearest neighbours through many routes, and a whole prepared scan compared with the
oracle only hopes that the rare ones occur in it.  Here every scan is built for named paths, and the test asserts, from
Context.search_report() of a context created under VGICP_DEBUG_PREP=1, that at least one query took each of them.

What every test does:
  1. a decoy first: a scan of the same size that shares no point with the real one is prepared on the same context, so
     that an output slot which no wave of the real preparation wrote holds a decoy value, not a correct stale one;
  2. the real scan on the debug context: kept indices and points equal to the oracle's, covariances bit for bit
     (test_gpu_parity._assert_preprocess_parity), through vgicp_preprocess and through vgicp_scan_prepare;
  3. the path counts named for the construction are > 0, and kept / n_heavy / n_light are the numpy count's;
  4. the same scan on a plain context (the kernel with debug == 0, as production runs it), after a decoy: equal bits.

When this module was written the kernel passed all of it: no bug found.  That the scans can tell was checked with
builds of the kernel made wrong on purpose, each of which fails here: ties in the re-ranking broken by the higher index
(both tied bands), a spilled cell left unmeasured (shell), the 27-cell block without its cells at the grid's upper or
lower edge (grid_edge: only its clusters across y = 0, whose neighbours lie in other edge cells than the query's own)."""
import numpy as np
import pytest

import knn_paths_reference as kp
from test_gpu_parity import _assert_preprocess_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def debug_ctx():
    """One context created under VGICP_DEBUG_PREP=1 (read when a context is created) for the whole module: every scan
    here meets the output slots and the counters that the scans before it left."""
    from eskf_lio_amd import capi
    with pytest.MonkeyPatch.context() as monkeypatch:
        monkeypatch.setenv("VGICP_DEBUG_PREP", "1")
        ctx = capi.Context(0)
        monkeypatch.delenv("VGICP_DEBUG_PREP")
    yield ctx
    ctx.close()


def _band(cfg):
    return kp.tied_band(**cfg)[0]


# name -> (scan, voxel size, knn, the paths at least one query must take)
CONSTRUCTIONS = {
    "shell": (kp.shell, kp.VOXEL, kp.KNN, ("spilled", "compacted", "open2", "leaf", "crowded")),
    "blob": (kp.blob, kp.VOXEL, kp.KNN, ("open1", "finest", "crowded")),
    "band_home": (lambda: _band(kp.BAND_HOME), kp.VOXEL, kp.KNN, ("home", "reranked")),
    "band_far": (lambda: _band(kp.BAND_FAR), kp.VOXEL, kp.KNN, ("reranked", "waited", "leaf")),
    "far_clusters": (kp.far_clusters, kp.VOXEL, kp.KNN, ("whole_scan", "no_own_cell")),
    "pile": (kp.pile, kp.VOXEL, kp.KNN, ("crowded", "finest")),
    "exactly_30": (lambda: kp.exactly(30), kp.VOXEL, kp.KNN, ("window_is_k",)),
    "exactly_17": (lambda: kp.exactly(17), kp.VOXEL, kp.KNN, ("window_is_k",)),
    "grid_edge": (kp.grid_edge, kp.EDGE_VOXEL, kp.KNN, ("clipped", "home")),
}
_REFERENCE = {}


def reference(oracle, key, scan, voxel, knn):
    """oracle.preprocess of a scan, computed once."""
    if key not in _REFERENCE:
        _REFERENCE[key] = oracle.preprocess(scan, voxel, knn)
    return _REFERENCE[key]


def after_decoy(ctx, scan, voxel, knn, seed, need):
    """vgicp_preprocess of a decoy, then of the scan.  The decoy keeps at least `need` points: it has written every
    output slot the scan's preparation is to write."""
    dp, dc, di = ctx.preprocess(kp.decoy(len(scan), seed, voxel), voxel, knn)
    assert len(di) >= need
    return ctx.preprocess(scan, voxel, knn)


def resident_after_decoy(ctx, scan, voxel, knn, seed):
    """The same through vgicp_scan_prepare / vgicp_scan_download (the resident scan's buffers)."""
    ctx.scan_prepare(kp.decoy(len(scan), seed, voxel), None, None, None, voxel, knn)
    kept, _ = ctx.scan_prepare(scan, None, None, None, voxel, knn)
    gp, gc = ctx.scan_download()
    return kept, gp, gc


def check(what, scan, voxel, knn, paths, debug_ctx, gpu_ctx, oracle, seed):
    ref = reference(oracle, what, scan, voxel, knn)
    m = len(ref[2])
    heavy, light = kp.heavy_light(scan, voxel)
    got = after_decoy(debug_ctx, scan, voxel, knn, seed, m)
    report = debug_ctx.search_report()
    print(f"[knn paths] {what}: {report.line()}")
    _assert_preprocess_parity(got, ref, scan)
    assert (report.kept, report.n_heavy, report.n_light) == (m, heavy, light), what
    for name in paths:
        assert getattr(report, name) > 0, (what, name, report.line())
    kept, gp, gc = resident_after_decoy(debug_ctx, scan, voxel, knn, seed + 1)
    assert kept == m and np.array_equal(gp, ref[0]) and np.array_equal(gc, ref[1]), what
    assert debug_ctx.search_report().paths() == report.paths(), what
    # production: a context created without the variable runs the kernel with debug == 0
    plain = after_decoy(gpu_ctx, scan, voxel, knn, seed + 2, m)
    for a, b in zip(plain, got):
        assert np.array_equal(a, b), what
    lists = gpu_ctx.search_report(start_lists_only=True)
    assert (lists.kept, lists.n_heavy, lists.n_light) == (m, heavy, light) and not any(lists.paths().values()), what
    return report


@pytest.mark.parametrize("what", sorted(CONSTRUCTIONS))
def test_scan_built_for_its_paths(debug_ctx, gpu_ctx, oracle, what):
    """Each construction of knn_paths_reference.py: oracle bits after a decoy on the debug context (both entry points),
    the named path counts > 0, the same bits from a plain context.  The report line is printed."""
    make, voxel, knn, paths = CONSTRUCTIONS[what]
    check(what, make(), voxel, knn, paths, debug_ctx, gpu_ctx, oracle, seed=sorted(CONSTRUCTIONS).index(what) * 10)


def test_every_path_has_a_construction():
    """The fourteen path counts of the report are each asserted > 0 by a construction above; a path added to the struct
    later without a scan built for it fails here."""
    from eskf_lio_amd import capi
    asserted = {name for _, _, _, paths in CONSTRUCTIONS.values() for name in paths}
    fields = [name for name, _ in capi.SearchReport._fields_]
    assert asserted == set(capi.SEARCH_PATHS) == set(kp.PATHS) == set(fields[10:]) and len(fields) == 24


def test_the_tied_bands_neighbours_are_decided_by_index(debug_ctx, oracle):
    """Tie-breaking inside the re-ranking, spelt out: the 30 nearest of the band's query are the query, the 20 near
    points, the 4 just inside the tie radius and the 5 exact ties of LOWEST index; the query's covariance is the
    oracle's covariance of exactly those 30 points given as a scan of their own (one voxel, k = 30 = n)."""
    for cfg in (kp.BAND_HOME, kp.BAND_FAR):
        scan, info = kp.tied_band(**cfg)
        d2 = kp.kernel_d2(scan, info["query"])
        order = np.lexsort((np.arange(len(scan)), d2))[:kp.KNN]
        assert (info["kind"][order] == 1).sum() == 5 and d2[order[-1]] == info["tie_d2"]
        ties = np.flatnonzero(info["kind"] == 1)
        assert set(order[info["kind"][order] == 1]) == set(ties[:5])
        dp, dc, di = debug_ctx.preprocess(kp.decoy(len(scan), 99, kp.VOXEL), kp.VOXEL, kp.KNN)
        gp, gc, gi = debug_ctx.preprocess(scan, kp.VOXEL, kp.KNN)
        assert gi[0] == 0
        # the 30 alone, the query first (so that it is the kept point of a voxel): its covariance from these 30
        chosen = scan[np.sort(order)]
        rp, rc, ri = oracle.preprocess(chosen, kp.VOXEL, kp.KNN)
        assert ri[0] == 0 and np.array_equal(gc[0], rc[0])
        # ... and not from the 30 with the tie of next-lowest index in place of the highest chosen one
        swapped = order.copy()
        swapped[-1] = ties[5]
        wp, wc, wi = oracle.preprocess(scan[np.sort(swapped)], kp.VOXEL, kp.KNN)
        assert not np.array_equal(wc[0], rc[0])


def test_one_cell_beyond_the_grid_is_refused(debug_ctx, gpu_ctx):
    """The grid-edge scan lies in the outermost finest cells and is accepted (test_scan_built_for_its_paths); with one
    coordinate in the first cell past the edge it is refused, on either context, and leaves no settled preparation."""
    from eskf_lio_amd import capi
    scan = kp.one_cell_beyond(kp.grid_edge())
    for ctx in (debug_ctx, gpu_ctx):
        with pytest.raises(capi.VgicpError) as e:
            ctx.preprocess(scan, kp.EDGE_VOXEL, kp.KNN)
        assert e.value.code == capi.ERR_BAD_ARGUMENT and "search grid" in str(e.value)
        with pytest.raises(capi.VgicpError) as e:
            ctx.search_report()
        assert e.value.code == capi.ERR_NOT_READY


def test_report_is_refused_without_the_variable_and_before_a_preparation(gpu_ctx, monkeypatch):
    from eskf_lio_amd import capi
    with pytest.raises(capi.VgicpError) as e:
        gpu_ctx.search_report()
    assert e.value.code == capi.ERR_NOT_READY
    monkeypatch.setenv("VGICP_DEBUG_PREP", "1")
    with capi.Context(0) as fresh:
        monkeypatch.delenv("VGICP_DEBUG_PREP")
        with pytest.raises(capi.VgicpError) as e:
            fresh.search_report()
        assert e.value.code == capi.ERR_NOT_READY
        fresh.preprocess(kp.exactly(17), kp.VOXEL, kp.KNN)
        report = fresh.search_report()
        assert report.window_is_k == report.kept > 0
    gpu_ctx.preprocess(kp.exactly(17), kp.VOXEL, kp.KNN)
    with pytest.raises(capi.VgicpError) as e:
        gpu_ctx.search_report()
    assert e.value.code == capi.ERR_BAD_ARGUMENT and "VGICP_DEBUG_PREP" in str(e.value)
    lists = gpu_ctx.search_report(start_lists_only=True)
    assert (lists.kept, lists.n_heavy + lists.n_light) == (17, 17)


# ---- the two start lists and their dispatch --------------------------------------------------------------------------
MIXED = [(n_light, n_heavy) for n_light in (8, 9, 15) for n_heavy in kp.MIXED_HEAVY] + [(63, 7), (64, 9), (65, 1)]


def check_start_lists(what, scan, n_heavy, n_light, debug_ctx, gpu_ctx, oracle, seed):
    n = len(scan)
    assert n == n_heavy + n_light and kp.heavy_light(scan) == (n_heavy, n_light)
    report = check(what, scan, kp.VOXEL, kp.KNN, (), debug_ctx, gpu_ctx, oracle, seed)
    assert (report.kept, report.n_heavy, report.n_light) == (n, n_heavy, n_light), what


@pytest.mark.parametrize("n", kp.START_SIZES)
def test_start_lists_all_heavy(debug_ctx, gpu_ctx, oracle, n):
    """n lonely points, each a voxel and a query of the heavy list: head = n rounded up to 8 waves, no light list."""
    check_start_lists(f"heavy {n}", kp.all_heavy(n), n, 0, debug_ctx, gpu_ctx, oracle, 200 + n)


@pytest.mark.parametrize("n", kp.LIGHT_SIZES)
def test_start_lists_all_light(debug_ctx, gpu_ctx, oracle, n):
    """n lattice points whose level-4 cells hold at least 4 points each: no heavy list (head = 0), the light list dealt
    over the 8 XCDs in shares of ceil(n / 8).  (1, 7 and 17 have no such block: knn_paths_reference.all_light.)"""
    check_start_lists(f"light {n}", kp.all_light(n), 0, n, debug_ctx, gpu_ctx, oracle, 400 + n)


@pytest.mark.parametrize("n_light,n_heavy", MIXED)
def test_start_lists_mixed(debug_ctx, gpu_ctx, oracle, n_light, n_heavy):
    """The light block and 1, 7 or 9 lonely points: head rounds 1 and 7 up to 8 and 9 up to 16, and the light list's
    length leaves 0, 1 and 7 queries over a multiple of 8."""
    assert {a % 8 for a, _ in MIXED} == {0, 1, 7}
    check_start_lists(f"mixed {n_light}+{n_heavy}", kp.mixed(n_light, n_heavy), n_heavy, n_light, debug_ctx, gpu_ctx,
                      oracle, 600 + 10 * n_light + n_heavy)
