"""vgicp_map_insert_resident_gated, its _async form and vgicp_map_gated_totals (include/vgicp_hip_map_gated.h): the
resident scan inserted into the map without the points a gate on d^2 rejects.

The rule is the header's, restated in tests/map_gated_reference.py and applied to what vgicp_points_resident returned at
the same pose just before the call; the map that results is held against a twin context that received the kept subset
through vgicp_map_insert_scan, and against the CPU oracle's LocalMap.  Every comparison is bit for bit.  The scenes'
preconditions are checked on the reference alone in tests/test_map_gated_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import map_gated_reference as mg
import robust_reference as rr
from map_gated_reference import GATES, MATCHED, NEGATIVE, NOT_FINITE, SIZES
from test_align_batch import assert_same_bits

pytestmark = pytest.mark.gpu

COUNTER_SCAN_GENERATION = 5
INF = float("inf")


@pytest.fixture(scope="module")
def scene():
    vmap, pts, covs, T_true, guess = rr.make_scene()
    return vmap, pts, covs, T_true, guess


@pytest.fixture(scope="module")
def prepared(oracle):
    """The lists route's two scans as the scan preparation leaves them (the oracle's preprocess: the device returns its
    bits, which the test asserts before it relies on them)."""
    raw_a, raw_b = mg.lidar_pair()
    return raw_a, raw_b, oracle.preprocess(raw_a, mg.PREP_VOXEL, 30)[:2], oracle.preprocess(raw_b, mg.PREP_VOXEL, 30)[:2]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def state(ctx, raw):
    """map_export, and with the raw-point store map_points_export, each sorted by key (stable: a voxel's points keep
    their insertion order)."""
    out = list(ctx.map_export())
    if raw:
        pk, pp = ctx.map_points_export()
        order = np.lexsort(pk.T)
        out += [pk[order], pp[order]]
    return out


def same_state(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def fresh(capi, voxel, raw, hint=0):
    ctx = capi.Context(0)
    if raw:
        ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
    ctx.map_reset(voxel, hint)
    return ctx


def build(ctx, vmap, cap=20):
    ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0])
    p, c, T = mg.first_scan(vmap)
    assert ctx.map_insert_scan(p, c, T, cap) == vmap.keys.shape[0]


def gated(ctx, pose, cap, gate):
    """The report at the pose, then the gated insertion: (kept, stats, report); the mask and the counts are checked
    against the rule on the way."""
    rep = ctx.points_resident(pose)
    kept, st = ctx.map_insert_resident_gated(pose, cap, gate)
    want = mg.rule(rep.d2, rep.status, gate)
    assert same_bits(kept, want), (gate, int(np.count_nonzero(kept != want)))
    assert (st.points, st.matched, st.refused, st.not_finite) == (rep.points,) + mg.counts(rep.status, want)
    return kept, st, rep


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_mask_is_the_rule_on_the_report(gpu_ctx, scene, n):
    vmap, pts, covs, T_true, _ = scene
    for gate in GATES:
        build(gpu_ctx, vmap)
        gpu_ctx.scan_upload(pts[:n], covs[:n])
        kept, st, rep = gated(gpu_ctx, T_true, 20, gate)
        assert len(kept) == n == st.points and st.launches >= 3 and st.device_seconds > 0.0
        if gate == INF:
            assert kept.all() and st.refused == 0
        if gate == 0.04 and n == 6000:   # the test cannot pass with an empty refusal set
            assert 0 < st.refused < st.matched < n and 0 < int(kept.sum()) < n
            print(f"n {n} gate {gate}: matched {st.matched} refused {st.refused} new voxels {st.new_voxels} "
                  f"launches {st.launches} device {1e6 * st.device_seconds:.1f} us")


# ---- 2 -------------------------------------------------------------------------------------------------------------
def run_route(capi, oracle, scene, prepared, route, raw, cap, gate=None):
    """A gated insertion on one context, the kept subset through vgicp_map_insert_scan on a twin, the same subset into
    the oracle: (state, twin state, oracle export, stats, twin's new voxels, kept, scan points)."""
    if route == "sort":
        vmap, pts, covs, pose, _ = scene
        voxel, gate = vmap.voxel_size, 0.04 if gate is None else gate
        first_p, first_c, first_T = mg.first_scan(vmap)
    else:
        raw_a, raw_b, (first_p, first_c), (pts, covs) = prepared
        voxel, pose, first_T = mg.MAP_VOXEL, np.eye(4), np.eye(4)
    with fresh(capi, voxel, raw, len(first_p)) as ctx, fresh(capi, voxel, raw, len(first_p)) as twin:
        if route == "sort":
            for c in (ctx, twin):
                c.map_insert_scan(first_p, first_c, first_T, cap)
            ctx.scan_upload(pts, covs)
        else:
            for c in (ctx, twin):
                c.scan_prepare(raw_a, None, None, None, mg.PREP_VOXEL, 30)
                c.map_insert_resident(first_T, cap)
            gp, gc = ctx.scan_download()
            assert same_bits(gp, first_p) and same_bits(gc, first_c)
            ctx.scan_prepare(raw_b, None, None, None, mg.PREP_VOXEL, 30)
            gp, gc = ctx.scan_download()
            assert same_bits(gp, pts) and same_bits(gc, covs)
            if gate is None:     # the 0.9 quantile of the ranked d^2: a tenth refused, lists of nine and ten points stay
                gate = float(ctx.points_resident(pose, [0.9], d2=False, sq_error=False, weight=False, status=False).quantiles[0])
        kept, st, rep = gated(ctx, pose, cap, gate)
        sel = kept.astype(bool)
        twin_new = twin.map_insert_scan(pts[sel], covs[sel], pose, cap)
        om = oracle.OracleMap(voxel, cap)
        om.insert(*oracle.transform(first_p, first_c, first_T))
        om.insert(*oracle.transform(pts[sel], covs[sel], pose))
        return state(ctx, raw), state(twin, raw), mg.sorted_oracle_export(om), st, twin_new, kept, pts


@pytest.mark.parametrize("cap", [1, 2, 20])
@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
@pytest.mark.parametrize("route", ["sort", "lists"])
def test_map_equals_the_kept_subset_inserted(oracle, scene, prepared, route, raw, cap):
    from eskf_lio_amd import capi
    got, twin, want, st, twin_new, kept, pts = run_route(capi, oracle, scene, prepared, route, raw, cap)
    assert 0 < st.refused < st.matched and st.new_voxels == twin_new
    if route == "lists":   # some voxel's list is longer than one chunk of the walk
        assert mg.per_voxel_counts(pts[kept.astype(bool)], mg.MAP_VOXEL).max() > mg.LIST_CHUNK
        assert st.launches == 3                      # decide, prepare, apply: no sort
    else:
        assert st.launches > 3
    assert same_state(got, twin), [same_bits(x, y) for x, y in zip(got, twin)]
    assert all(same_bits(x, y) for x, y in zip(got[:4], want)), [same_bits(x, y) for x, y in zip(got[:4], want)]
    if raw:
        assert len(got[5]) == int(got[3].sum())


# ---- 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["sort", "lists"])
def test_order_inside_a_voxel(route):
    """Twelve points into one voxel that exists, alternately within and beyond the gate: the record and the raw ordinals
    are those of the six kept points inserted alone."""
    from eskf_lio_amd import capi
    first, first_c, pts, covs = mg.crafted_voxel()
    gate = 1.0 if route == "sort" else 0.02
    with fresh(capi, mg.MAP_VOXEL, True) as ctx, fresh(capi, mg.MAP_VOXEL, True) as twin:
        for c in (ctx, twin):
            c.map_insert_scan(first, first_c, np.eye(4), 20)
        if route == "sort":
            ctx.scan_upload(pts, covs)
        else:
            ctx.scan_prepare(pts, None, None, None, mg.PREP_VOXEL, 30)
            got_p, covs = ctx.scan_download()
            assert same_bits(got_p[:12], pts[:12])   # twelve cells of the 0.1 grid, in scan order (some filler shares cells)
            pts = got_p
        kept, st, rep = gated(ctx, np.eye(4), 20, gate)
        assert kept[:12].tolist() == [1, 0] * 6 and kept[12:].all() and np.all(rep.status[:12] == MATCHED)
        assert not rep.status[12:].any() and st.refused == 6 and st.new_voxels > 0
        sel = kept.astype(bool)
        assert twin.map_insert_scan(pts[sel], covs[sel], np.eye(4), 20) == st.new_voxels
        a, b = state(ctx, True), state(twin, True)
        assert same_state(a, b)
        here = np.all(a[4] == 0, axis=1)
        assert same_bits(a[5][here], np.vstack([first, pts[:12:2]]))          # the ordinals: 3 founders, then scan order
        assert int(a[3][np.all(a[0] == 0, axis=1)][0]) == 9


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_nothing_kept_and_everything_kept(scene):
    from eskf_lio_amd import capi
    vmap, pts, covs, T_true, _ = scene
    with fresh(capi, vmap.voxel_size, True) as ctx, fresh(capi, vmap.voxel_size, True) as twin:
        for c in (ctx, twin):
            c.map_insert_scan(*mg.first_scan(vmap), 20)
        ctx.scan_upload(pts, covs)
        rep = ctx.points_resident(T_true)
        all_matched = (rep.status & MATCHED) != 0
        p, c = pts[all_matched], covs[all_matched]
        ctx.scan_upload(p, c)
        rep = ctx.points_resident(T_true)
        assert rep.matched == rep.points == len(p) and rep.d2.min() > 0.0
        before = state(ctx, True)
        kept, st, _ = gated(ctx, T_true, 20, float(rep.d2.min()) / 2.0)
        assert not kept.any() and st.refused == len(p) and st.new_voxels == 0
        assert same_state(state(ctx, True), before)
        # everything kept: vgicp_map_insert_resident on a twin
        ctx.scan_upload(pts, covs)
        twin.scan_upload(pts, covs)
        kept, st, _ = gated(ctx, T_true, 20, INF)
        assert kept.all() and st.refused == 0
        assert twin.map_insert_resident(T_true, 20) == st.new_voxels > 0
        assert same_state(state(ctx, True), state(twin, True))


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_flags(gpu_ctx, scene):
    """A NaN covariance (raw not finite) is refused at every gate, +inf included; an indefinite one (raw < 0) counts as
    d^2 = 0 and is kept at gate 0.  Crafted as tests/test_points.py crafts them."""
    vmap, pts, covs, T_true, _ = scene
    n = 300
    build(gpu_ctx, vmap)
    gpu_ctx.scan_upload(pts[:n], covs[:n])
    matched = np.flatnonzero(gpu_ctx.points_resident(T_true).status & MATCHED)
    a, b = int(matched[3]), int(matched[40])
    lam = float(np.linalg.eigvalsh(vmap.covs.reshape(-1, 3, 3)).max())
    edited = covs[:n].copy()
    edited[a] = np.nan
    edited[b] = (-4.0 * max(1.0, lam) * np.eye(3)).reshape(9)
    for gate in (0.0, 0.04, INF):
        build(gpu_ctx, vmap)
        gpu_ctx.scan_upload(pts[:n], edited)
        kept, st, rep = gated(gpu_ctx, T_true, 20, gate)
        assert rep.status[a] == MATCHED | NOT_FINITE and rep.status[b] == MATCHED | NEGATIVE
        assert kept[a] == 0 and kept[b] == 1 and st.not_finite == 1, gate
        if gate == INF:
            assert st.refused == 1
        if gate == 0.0:
            assert int(kept[matched].sum()) == 1          # every other matched point has d^2 > 0


# ---- 6 -------------------------------------------------------------------------------------------------------------
def frame_poses(T_true):
    out = []
    for f in range(3):
        T = np.array(T_true)
        T[:3, 3] += 0.01 * f
        out.append(T)
    return out


@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
def test_async_gives_the_sync_map_and_the_totals(scene, raw):
    from eskf_lio_amd import capi
    vmap, pts, covs, T_true, _ = scene
    with fresh(capi, vmap.voxel_size, raw) as sync, fresh(capi, vmap.voxel_size, raw) as deferred:
        for c in (sync, deferred):
            c.map_insert_scan(*mg.first_scan(vmap), 20)
            c.scan_upload(pts, covs)
            assert c.map_gated_totals() == (0, 0)
        points = refused = 0
        for T in frame_poses(T_true):
            _, st = sync.map_insert_resident_gated(T, 20, 0.04, kept=False)
            points, refused = points + st.points, refused + st.refused
            deferred.frame_stats(reset=True)
            deferred.map_insert_resident_gated_async(T, 20, 0.04)
        assert refused > 0 and points == 3 * len(pts)
        assert deferred.map_gated_totals() == sync.map_gated_totals() == (points, refused)
        assert same_state(state(deferred, raw), state(sync, raw))
        assert deferred.map_size()[0] == sync.map_size()[0]
        deferred.map_reset(vmap.voxel_size, 0)
        assert deferred.map_gated_totals() == (0, 0) and sync.map_gated_totals() == (points, refused)


def test_async_waits_for_nothing(scene):
    """The first deferred call finds nothing pending and synchronises not at all; a second settles the first (one)."""
    from eskf_lio_amd import capi
    vmap, pts, covs, T_true, _ = scene
    with fresh(capi, vmap.voxel_size, False, 4 * len(vmap.keys)) as ctx:
        ctx.map_insert_scan(*mg.first_scan(vmap), 20)
        ctx.scan_upload(pts, covs)
        ctx.frame_stats(reset=True)
        ctx.map_insert_resident_gated_async(T_true, 20, 0.04)
        assert ctx.frame_stats().host_syncs == 0
        ctx.map_insert_resident_gated_async(T_true, 20, 0.04)
        assert ctx.frame_stats().host_syncs == 1


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_afterwards_the_twin_bits(scene):
    """An align (which builds the dense copy and the memos) before the insertion, and an align, an evaluation and a report
    after it: the bits of a twin whose map received the kept subset."""
    from eskf_lio_amd import capi
    vmap, pts, covs, T_true, guess = scene
    with fresh(capi, vmap.voxel_size, False) as ctx, fresh(capi, vmap.voxel_size, False) as twin:
        for c in (ctx, twin):
            c.map_insert_scan(*mg.first_scan(vmap), 20)
            c.scan_upload(pts, covs)
            c.align_resident(guess, rr.MAX_IT, rr.TSQ, rr.COS)
        kept, _, _ = gated(ctx, T_true, 20, 0.04)
        sel = kept.astype(bool)
        twin.map_insert_scan(pts[sel], covs[sel], T_true, 20)
        for flags in (0, capi.FLAG_NO_PERSISTENT):
            assert_same_bits(ctx.align_resident(guess, rr.MAX_IT, rr.TSQ, rr.COS, flags=flags),
                             twin.align_resident(guess, rr.MAX_IT, rr.TSQ, rr.COS, flags=flags), f"flags {flags}")
        for g, w in zip(ctx.evaluate_resident([guess, T_true]), twin.evaluate_resident([guess, T_true])):
            assert g.correspondences == w.correspondences and g.cost == w.cost and g.sq_error == w.sq_error
            assert same_bits(g.normal_eq, w.normal_eq)
        a, b = ctx.points_resident(T_true, [0.5]), twin.points_resident(T_true, [0.5])
        assert all(same_bits(x, y) for x, y in ((a.d2, b.d2), (a.sq_error, b.sq_error), (a.weight, b.weight),
                                                (a.status, b.status), (a.quantiles, b.quantiles)))
        assert ctx.counter(1) == 0 and twin.counter(1) == 0


# ---- 8 -------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order(scene):
    from eskf_lio_amd import capi
    vmap, pts, covs, T_true, _ = scene
    lib = capi.load_library()
    n = len(pts)
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    good = capi.pose_to_abi(T_true)
    bad = good.copy()
    bad[13] = np.inf
    kept = np.full(n, 0xA5, dtype=np.uint8)
    stats = capi.GatedInsertStats()

    def sync(ctx, pose=good, cap=20, gate=0.04, capacity=n, with_kept=True):
        C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
        kept[:] = 0xA5
        return lib.vgicp_map_insert_resident_gated(ctx._h if ctx is not None else None,
                                                   pose.ctypes.data_as(dp) if pose is not None else None, cap, gate,
                                                   capacity, kept.ctypes.data_as(u8p) if with_kept else None, C.byref(stats))

    def deferred(ctx, pose=good, cap=20, gate=0.04, **_):
        C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
        kept[:] = 0xA5
        return lib.vgicp_map_insert_resident_gated_async(ctx._h if ctx is not None else None,
                                                         pose.ctypes.data_as(dp) if pose is not None else None, cap, gate)

    def untouched():
        return np.all(kept == 0xA5) and bytes(stats) == b"\xa5" * C.sizeof(stats)

    for call in (sync, deferred):
        assert call(None) == capi.ERR_BAD_ARGUMENT and untouched()                                      # 1
        assert lib.vgicp_map_gated_totals(None, None, None) == capi.ERR_BAD_ARGUMENT
        with capi.Context(0) as ctx:
            # 3: plan_insert's order, each in front of everything behind it
            assert call(ctx, pose=None, cap=0, gate=np.nan) == capi.ERR_NOT_READY and "map" in ctx.last_error()
            ctx.map_reset(vmap.voxel_size, len(vmap.keys))
            ctx.map_insert_scan(*mg.first_scan(vmap), 20)
            assert call(ctx, pose=None, cap=0, gate=np.nan) == capi.ERR_NOT_READY and "scan" in ctx.last_error()
            ctx.scan_upload(pts, covs)
            before, generation = state(ctx, False), ctx.counter(COUNTER_SCAN_GENERATION)

            def refused(text, writes_points=False, **kwargs):
                assert call(ctx, **kwargs) == capi.ERR_BAD_ARGUMENT and text in ctx.last_error(), (kwargs, ctx.last_error())
                assert writes_points or untouched()
                assert same_state(state(ctx, False), before) and ctx.counter(COUNTER_SCAN_GENERATION) == generation

            refused("NULL pointer", pose=None, cap=0, gate=np.nan)
            refused("max_points_per_voxel", pose=bad, cap=0, gate=np.nan)
            refused("not finite", pose=bad, gate=np.nan)                                                 # 4 before 5
            for gate in (np.nan, -1.0, -INF, -1e-300):                                                   # 5
                refused("gate must be", gate=gate, capacity=0)
            # a communicator (one rank is enough): the resident scan counts as a shard there, which plan_insert refuses
            # with the resident entries' own text before rule 6 is reached
            ctx.comm_init(1, 0, ctx.comm_unique_id())
            refused("resident scan is a shard")
            refused("resident scan is a shard", gate=np.nan)
            ctx.comm_destroy()
            if call is sync:                                                                             # 7
                refused("kept holds fewer", writes_points=True, capacity=n - 1)
                assert stats.points == n and np.all(kept == 0xA5) and bytes(stats)[8:] == b"\xa5" * (C.sizeof(stats) - 8)
                assert call(ctx, capacity=0, with_kept=False) == capi.OK and np.all(kept == 0xA5) and stats.points == n
            else:
                assert call(ctx) == capi.OK
            assert not same_state(state(ctx, False), before)
        with capi.Context(0) as ctx:                                   # the raw-point store's bound is plan_insert's too
            ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
            ctx.map_reset(vmap.voxel_size, 0)
            ctx.scan_upload(pts, covs)
            assert call(ctx, pose=bad, cap=2 ** 32) == capi.ERR_BAD_ARGUMENT and "2^32" in ctx.last_error()
        with capi.Context([0, 0]) as multi:                                                              # 6
            assert call(multi) == capi.ERR_NOT_READY                     # 3 before 6: no map
            multi.map_reset(vmap.voxel_size, len(vmap.keys))
            multi.map_upsert(vmap.keys, vmap.means, vmap.covs)
            multi.scan_upload(pts, covs)
            before = state(multi, False)
            assert call(multi, gate=-1.0) == capi.ERR_BAD_ARGUMENT and "gate must be" in multi.last_error()   # 5 before 6
            assert call(multi) == capi.ERR_BAD_ARGUMENT and "single-device" in multi.last_error() and untouched()
            assert call(multi, capacity=0) == capi.ERR_BAD_ARGUMENT and "single-device" in multi.last_error()   # 6 before 7
            assert same_state(state(multi, False), before)
            assert multi.map_gated_totals() == (0, 0)


# ---- 9 -------------------------------------------------------------------------------------------------------------
def test_the_point_of_it(oracle, scene):
    """Ten frames of a static scene plus a displaced cluster (tests/map_gated_reference.make_chain: selected on the
    reference alone, the gate a factor of two from either class).  The gated chain's final map is, bit for bit, the map
    of the chain fed only the static points, and the oracle's; the plain chain's is not."""
    from eskf_lio_amd import capi
    vmap = scene[0]
    frames, om = mg.make_chain(oracle, vmap)
    with fresh(capi, vmap.voxel_size, True) as gate_ctx, fresh(capi, vmap.voxel_size, True) as static_ctx, \
            fresh(capi, vmap.voxel_size, True) as plain_ctx:
        for c in (gate_ctx, static_ctx, plain_ctx):
            c.map_insert_scan(*mg.first_scan(vmap), mg.CHAIN_CAP)
        refused = 0
        for f, (pts, covs, T, moved, _) in enumerate(frames):
            gate_ctx.scan_upload(pts, covs)
            if f % 2:     # both forms along the chain
                gate_ctx.map_insert_resident_gated_async(T, mg.CHAIN_CAP, mg.CHAIN_GATE)
            else:
                kept, st = gate_ctx.map_insert_resident_gated(T, mg.CHAIN_CAP, mg.CHAIN_GATE)
                assert same_bits(kept, (~moved).astype(np.uint8)), f
            refused += int(moved.sum())
            static_ctx.scan_upload(pts[~moved], covs[~moved])
            static_ctx.map_insert_resident(T, mg.CHAIN_CAP)
            plain_ctx.scan_upload(pts, covs)
            plain_ctx.map_insert_resident(T, mg.CHAIN_CAP)
        assert gate_ctx.map_gated_totals() == (sum(len(fr[0]) for fr in frames), refused) and refused > 1000
        got, want, plain = state(gate_ctx, True), state(static_ctx, True), state(plain_ctx, True)
        assert same_state(got, want)
        assert all(same_bits(x, y) for x, y in zip(got[:4], mg.sorted_oracle_export(om)))
        assert not same_state(plain, want)
        assert same_bits(plain[0], want[0]) and not same_bits(plain[1], want[1])     # the same voxels, dragged means


# ---- the drop-in classes: LocalMap::setInsertGate on the frame path ---------------------------------------------------
def test_drop_in_frames_with_a_gate_end_at_the_abi_chain(tmp_path):
    """CloudPreprocessor::process -> ICP::align -> LocalMap::updateLocalMap through the C++ classes (host.Frame, written
    as src/Odometry.cpp:73-87 writes it) with LocalMap::setInsertGate: every update is the gated resident insertion, so
    poses, map, raw points and totals are bit for bit those of the C-ABI chain vgicp_scan_prepare_async ->
    vgicp_align_resident -> vgicp_map_insert_resident_gated_async on a context that keeps its raw points.  The map was
    built with the shadow grid (the default): setInsertGate moves the raw points to the device, and save() writes them."""
    from eskf_lio_amd import capi, host
    from test_multi_device import _NO_GATE, _frame_inputs
    st, t, ext, raws = _frame_inputs(frames=4, n=20_000)
    cap = 20
    # the gate: the 0.8 quantile of d^2 of the second frame against the first (a fifth of the matched points beyond it)
    with capi.Context(0) as c:
        c.map_reset(0.3, 0)
        c.scan_prepare_async(raws[0], None, None, ext, 0.3, 30)
        c.map_insert_resident_async(np.eye(4), cap)
        c.scan_prepare_async(raws[1], t, st, ext, 0.3, 30)
        pose = c.align_resident(np.eye(4), 30, 1e-6, 0.9999).pose
        gate = float(c.points_resident(pose, [0.8], d2=False, sq_error=False, weight=False, status=False).quantiles[0])
    assert gate > 0.0
    with capi.Context(0) as c:
        c.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
        c.map_reset(0.3, 0)
        pose, want = np.eye(4), []
        for f, raw in enumerate(raws):
            c.scan_prepare_async(raw, t if f else None, st if f else None, ext, 0.3, 30)
            if f > 0:
                r = c.align_resident(pose, 30, 1e-6, 0.9999)
                pose = r.pose
                want.append((r.pose, r.iterations))
            c.map_insert_resident_gated_async(pose, cap, gate)
        want_totals = c.map_gated_totals()
        want_state = state(c, True)
    assert 0 < want_totals[1] < want_totals[0]

    pre = host.CloudPreprocessor(0.3, ext, "deferred")
    icp = host.ICP(30, 1e-6, 0.9999)
    lmap = host.LocalMap(0.3, cap, dict(_NO_GATE, device_resident=True))            # keeps raw points, in the shadow grid
    assert lmap.insertGate() == 0.0 and lmap.gatedTotals() == (0, 0, 0)
    lmap.setInsertGate(gate)
    assert lmap.insertGate() == gate and lmap.savesRawPoints()
    pose = np.eye(4)
    for f, raw in enumerate(raws):
        fr = host.Frame(raw, t, st)
        fr.run(pre, icp, lmap, pose, first_frame=(f == 0), move_cloud=(f == 2))
        got = fr.end()
        if f == 0:
            continue
        pose = got["pose"]
        assert got["used_resident"] and got["iterations"] == want[f - 1][1]
        assert np.array_equal(pose, want[f - 1][0]), f
    assert lmap.gatedTotals() == want_totals + (0,)                               # no frame went in whole
    keys, means, covs, counts = lmap.export()
    order = np.lexsort(keys.T)
    assert all(same_bits(x, y) for x, y in zip((keys[order], means[order], covs[order], counts[order]), want_state[:4]))
    # save(): the raw points come from the device (the refused ones are not among them)
    pcd, traj = tmp_path / "map.pcd", tmp_path / "traj.json"
    lmap.save(str(pcd), str(traj))
    lines = pcd.read_text().splitlines()
    start = lines.index("DATA ascii") + 1
    saved = np.array([[float(v) for v in ln.split()] for ln in lines[start:]])
    assert saved.shape == want_state[5].shape == (int(want_state[3].sum()), 3)
    assert np.array_equal(saved[np.lexsort(saved.T)], want_state[5][np.lexsort(want_state[5].T)])
    # switching the gate off again: the next frame goes in whole, through the plain entry
    lmap.setInsertGate(0.0)
    fr = host.Frame(raws[1], t, st)
    fr.run(pre, icp, lmap, pose)
    fr.end()
    assert lmap.gatedTotals() == want_totals + (0,)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="setInsertGate"):
            lmap.setInsertGate(bad)
    # a map that already holds frames cannot move its raw points to the device: the gate is refused, the map stays as it is
    late = host.LocalMap(0.3, cap, dict(_NO_GATE, device_resident=True))
    fr = host.Frame(raws[0], t, st)
    fr.run(pre, icp, late, np.eye(4), first_frame=True)
    fr.end()
    with pytest.raises(ValueError):
        late.setInsertGate(gate)
    assert late.insertGate() == 0.0 and len(late) > 0
    with pytest.raises(ValueError, match="device-resident"):
        host.LocalMap(0.3, cap).setInsertGate(gate)


def test_kept_is_written_for_the_first_n_only(gpu_ctx, scene):
    """capacity > n: the first n entries of kept are written, the tail keeps the caller's bytes."""
    from eskf_lio_amd import capi
    vmap, pts, covs, T_true, _ = scene
    n, room = 300, 340
    lib = capi.load_library()
    build(gpu_ctx, vmap)
    gpu_ctx.scan_upload(pts[:n], covs[:n])
    rep = gpu_ctx.points_resident(T_true)
    kept = np.full(room, 0xA5, dtype=np.uint8)
    stats = capi.GatedInsertStats()
    pose = capi.pose_to_abi(T_true)
    rc = lib.vgicp_map_insert_resident_gated(gpu_ctx._h, pose.ctypes.data_as(C.POINTER(C.c_double)), 20, 0.04, room,
                                             kept.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(stats))
    assert rc == capi.OK and stats.points == n
    assert same_bits(kept[:n], mg.rule(rep.d2, rep.status, 0.04)) and np.all(kept[n:] == 0xA5)
    assert 0 < stats.refused < n


# ---- the replay on the resident chain ---------------------------------------------------------------------------------
def gated_config(replay, gate):
    return dict(replay.DEFAULT_CONFIG, local_map=dict(replay.DEFAULT_CONFIG["local_map"], insert_gate=gate))


def clone_events(replay, events):
    from replay_backends import stream_events
    return stream_events(replay, events)


@pytest.fixture(scope="module")
def stream():
    from eskf_lio_amd import synth
    return synth.make_sensor_stream(frames=4, points_per_frame=6_000)[0]


def test_replay_on_the_resident_chain(stream):
    """local_map.insert_gate on replay.DeviceBackend: at +inf (nothing finite is refused) trajectory and map are the plain
    chain's bit for bit; a finite gate refuses points and leaves another map."""
    from eskf_lio_amd import replay
    runs = {}
    for name, gate in (("plain", 0.0), ("inf", INF), ("gate", 0.04)):
        cfg = gated_config(replay, gate) if gate else replay.DEFAULT_CONFIG
        backend = replay.DeviceBackend(cfg, 0)
        traj = replay.Odometry(cfg, backend).run(clone_events(replay, stream))
        runs[name] = (traj, state(backend.ctx, False), backend.ctx.map_gated_totals())
        backend.ctx.close()
    assert len(runs["plain"][0]) == 4 and runs["plain"][2] == (0, 0)
    assert all(a[0] == b[0] and same_bits(a[1], b[1]) for a, b in zip(runs["plain"][0], runs["inf"][0]))
    assert same_state(runs["plain"][1], runs["inf"][1])
    assert runs["inf"][2][0] > 0 and runs["inf"][2][1] == 0
    points, refused = runs["gate"][2]
    assert 0 < refused < points
    assert not same_state(runs["gate"][1], runs["plain"][1])
