"""vgicp_map_carve_resident, its _async form and vgicp_map_carve_totals (include/vgicp_hip_map_carve.h): the voxels the
resident scan sees through, removed from the map on the device.

The rule is the header's, restated operation by operation in tests/map_carve_reference.py: the set of removed keys and
every count are compared exactly (the rule is written so that the device returns numpy's bits), and independently of the
operation order through the brute-force sandwich.  tests/test_map_carve_cpu.py checks the reference on its own."""
import ctypes as C

import numpy as np
import pytest

import map_carve_reference as mc
from map_carve_reference import MARGINS, MIN_HITS, ORIGIN, SIZES, STRIDES, VOXEL, Params

pytestmark = pytest.mark.gpu

COUNTER_SCAN_GENERATION = 5
CAP = 20


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def state(ctx, raw=False):
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


def without(st, keys):
    """A state with the voxels (and raw points) of `keys` taken out."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    keep = mc.match(keys, st[0]) < 0
    out = [a[keep] for a in st[:4]]
    if len(st) > 4:
        keep = mc.match(keys, st[4]) < 0
        out += [a[keep] for a in st[4:]]
    return out


def scan_covs(n):
    return np.tile((1e-3 * np.eye(3)).reshape(9), (n, 1))


@pytest.fixture(scope="module")
def vmap():
    from eskf_lio_amd import synth
    return synth.make_map(mc.MAP_VOXELS, voxel_size=VOXEL)


@pytest.fixture(scope="module")
def scene(vmap):
    """The largest scan; every smaller one is its head (a prefix of a scan is a scan)."""
    _, pts, T = mc.make_scene(max(SIZES), vmap=vmap)
    return pts, T


_walks = {}


def reference(vmap, pts, T, p: Params):
    """The reference's hits and shield for (scan, stride, margin), computed once; the decision at p.min_hits."""
    key = (len(pts), p.stride, p.margin, p.max_range, p.origin, pts.tobytes()[:64])
    if key not in _walks:
        _walks[key] = mc.carve(vmap.keys, VOXEL, pts, T, Params(p.margin, p.max_range, 1, p.stride, p.origin))
    res = _walks[key]
    return mc.Result(res.hits, res.shield, (res.hits >= p.min_hits) & ~res.shield, res.rays, res.visits, res.steps)


def load(ctx, vmap, hint=None):
    ctx.map_reset(vmap.voxel_size, len(vmap.keys) if hint is None else hint)
    ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)


def counts_of(st):
    return dict(rays=st.rays, visits=st.visits, touched=st.touched, shielded=st.shielded, removed=st.removed)


# ---- 1: parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_removed_keys_and_counts_are_the_references(gpu_ctx, vmap, scene, n):
    pts, T = scene[0][:n], scene[1]
    load(gpu_ctx, vmap)
    before = state(gpu_ctx)
    removed_somewhere = 0
    for stride in STRIDES:
        for margin in MARGINS:
            for min_hits in MIN_HITS:
                p = Params(margin=margin, min_hits=min_hits, stride=stride, origin=ORIGIN)
                want = reference(vmap, pts, T, p)
                load(gpu_ctx, vmap)
                gpu_ctx.scan_upload(pts, scan_covs(n))
                size0 = gpu_ctx.map_size()[0]
                keys, st = gpu_ctx.map_carve_resident(T, p.as_dict())
                what = (n, stride, margin, min_hits)
                assert same_bits(mc.sorted_keys(keys), mc.sorted_keys(vmap.keys[want.removed])), what
                assert counts_of(st) == want.counts(), (what, counts_of(st), want.counts())
                assert st.launches == 2 and st.device_seconds > 0.0
                assert gpu_ctx.map_size()[0] == size0 - st.removed
                assert same_state(state(gpu_ctx), without(before, keys)), what          # the survivors, bit for bit
                removed_somewhere += st.removed
    assert removed_somewhere > 0
    if n == max(SIZES):
        print(f"n {n}: {want.counts()} device {1e6 * st.device_seconds:.1f} us")


def test_keys_are_written_up_to_capacity_and_the_count_is_whole(gpu_ctx, vmap, scene):
    from eskf_lio_amd import capi
    pts, T = scene[0][:1000], scene[1]
    p = Params(origin=ORIGIN)
    want = reference(vmap, pts, T, p)
    total = int(want.removed.sum())
    assert total > 100
    lib = capi.load_library()
    pose, cp = capi.pose_to_abi(T), capi.carve_params(**p.as_dict())
    for capacity, with_keys in ((0, True), (7, True), (total, True), (total + 50, True), (0, False)):
        load(gpu_ctx, vmap)
        gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
        keys = np.full((total + 60, 3), 0x5A5A5A5A, dtype=np.int32)
        removed = C.c_size_t(0)
        rc = lib.vgicp_map_carve_resident(gpu_ctx._h, pose.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cp), capacity,
                                          keys.ctypes.data_as(C.POINTER(C.c_int32)) if with_keys else None, C.byref(removed), None)
        assert rc == capi.OK and removed.value == total and gpu_ctx.map_size()[0] == len(vmap.keys) - total
        m = min(capacity, total) if with_keys else 0
        assert np.all(keys[m:] == 0x5A5A5A5A)
        assert np.all(mc.match(vmap.keys[want.removed], keys[:m]) >= 0) and len(np.unique(keys[:m], axis=0)) == m


def test_raw_points_of_the_survivors_stay(vmap, scene):
    from eskf_lio_amd import capi
    pts, T = scene[0][:1000], scene[1]
    rng = np.random.default_rng(5)
    with capi.Context(0) as ctx:
        ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
        ctx.map_reset(VOXEL, len(vmap.keys))
        for f in range(2):       # two or one raw point per voxel, the first scan's first
            sel = np.arange(len(vmap.keys)) if f == 0 else np.flatnonzero(rng.random(len(vmap.keys)) < 0.5)
            p3 = (vmap.keys[sel] + rng.uniform(0.05, 0.95, size=(len(sel), 3))) * VOXEL
            ctx.map_insert_scan(p3, vmap.covs[sel], np.eye(4), CAP)
        before = state(ctx, True)
        assert len(before[0]) == len(vmap.keys) and len(before[5]) > len(vmap.keys)
        ctx.scan_upload(pts, scan_covs(len(pts)))
        p = Params(origin=ORIGIN, min_hits=2)
        keys, st = ctx.map_carve_resident(T, p.as_dict())
        want = reference(vmap, pts, T, p)
        assert same_bits(mc.sorted_keys(keys), mc.sorted_keys(vmap.keys[want.removed])) and st.removed > 100
        after = state(ctx, True)
        assert same_state(after, without(before, keys))
        assert len(after[5]) == int(after[3].sum()) < len(before[5])


# ---- 2: the sandwich on the device's result -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", mc.SCENE_SEEDS)
def test_device_result_lies_inside_the_sandwich(gpu_ctx, vmap, seed):
    _, pts, T = mc.make_scene(400, seed, vmap)
    for margin in MARGINS:
        p = Params(margin=margin, origin=ORIGIN)
        certain, possible = mc.slab_counts(vmap.keys, VOXEL, pts, T, p)
        shield = mc.carve(vmap.keys, VOXEL, pts, T, p).shield
        for min_hits in MIN_HITS:
            load(gpu_ctx, vmap)
            gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
            keys, st = gpu_ctx.map_carve_resident(T, dict(p.as_dict(), min_hits=min_hits))
            removed = np.zeros(len(vmap.keys), dtype=bool)
            removed[mc.match(vmap.keys, keys)] = True
            missed, wrong = mc.check_sandwich(removed, shield, certain, possible, min_hits)
            assert len(missed) == 0 and len(wrong) == 0 and st.removed == removed.sum() > 0, (seed, margin, min_hits)


# ---- 3: invariants ----------------------------------------------------------------------------------------------------
def test_a_voxel_that_holds_a_return_is_never_removed(gpu_ctx, vmap, scene):
    pts, T = scene
    ek, defined = mc.keys_of(mc.transform(T, pts), VOXEL)
    held = mc.match(vmap.keys, ek[defined])
    assert np.count_nonzero(held >= 0) > 500
    for stride in (1, 3, 64, len(pts) + 1):          # the shield is every point's, whatever the stride
        load(gpu_ctx, vmap)
        gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
        keys, st = gpu_ctx.map_carve_resident(T, Params(origin=ORIGIN, stride=stride).as_dict())
        assert st.removed > 0 and st.rays == len(range(0, len(pts), stride))
        assert np.all(mc.match(keys, ek[defined]) < 0)
        assert st.shielded > 0 or stride > 3          # (touched AND shielded: a single ray may meet no such voxel)


def test_a_second_call_is_the_reference_on_the_carved_map(gpu_ctx, scene):
    """On a sparse map (a ray meets a few voxels only): a second identical call is the reference run on the carved map.
    The walk does not stop at a FULL voxel, so the survivors' hits are what they were and nothing more goes."""
    from eskf_lio_amd import synth
    sparse = synth.make_map(2_000, voxel_size=VOXEL)
    pts, T = scene[0][:1000] * 0.5, scene[1]
    for min_hits in (1, 2):
        p = Params(origin=ORIGIN, min_hits=min_hits)
        load(gpu_ctx, sparse)
        gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
        first, st1 = gpu_ctx.map_carve_resident(T, p.as_dict())
        left = sparse.keys[mc.match(first, sparse.keys) < 0]
        want = mc.carve(left, VOXEL, pts, T, p)
        second, st2 = gpu_ctx.map_carve_resident(T, p.as_dict())
        assert st1.removed > 0 and same_bits(mc.sorted_keys(second), mc.sorted_keys(left[want.removed].astype(np.int32)))
        assert counts_of(st2) == want.counts() and st2.removed == 0 and st2.touched == st1.touched - st1.removed


@pytest.mark.parametrize("route", ["sort", "lists"])
def test_an_insertion_after_a_carve_is_the_insertion_after_an_erase(oracle, vmap, scene, route):
    """No mark is left in a record: the insertion that follows (which threads its lists through the same spare word) gives
    the map of a twin from which the same keys were erased by vgicp_map_erase, and the oracle's."""
    from eskf_lio_amd import capi, synth
    import map_gated_reference as mg
    pts, T = scene[0][:2000], scene[1]
    with capi.Context(0) as ctx, capi.Context(0) as twin:
        for c in (ctx, twin):
            c.map_reset(VOXEL, len(vmap.keys))
            c.map_insert_scan(*mg.first_scan(vmap), CAP)
        if route == "sort":
            covs = synth.disc_covariances(3, 16, np.arange(len(pts), dtype=np.uint64))
            for c in (ctx, twin):
                c.scan_upload(pts, covs)
        else:             # a scan the device prepared itself: the insertion goes without its sort
            raw = synth.make_lidar_scan(6_000, seed=4, extent=12.0)
            for c in (ctx, twin):
                c.scan_prepare(raw, None, None, None, 0.3, 30)
            pts, covs = ctx.scan_download()
        keys, st = ctx.map_carve_resident(T, Params(origin=ORIGIN, min_hits=2).as_dict())
        assert st.removed > 100
        twin.map_erase(keys)
        launches = []
        for c in (ctx, twin):
            c.frame_stats(reset=True)
            c.map_insert_resident(T, CAP)
            launches.append(c.frame_stats().kernel_launches)
        assert launches[0] == launches[1] and (launches[0] == 2) == (route == "lists")
        got, want = state(ctx), state(twin)
        assert same_state(got, want)
        # the oracle: the survivors as they were, then the scan
        left = mc.match(keys, vmap.keys) < 0
        om = oracle.OracleMap(VOXEL, CAP)
        om.insert(vmap.means[left], vmap.covs[left])
        om.insert(*oracle.transform(pts, covs, T))
        assert all(same_bits(x, y) for x, y in zip(got, mg.sorted_oracle_export(om)))


# ---- 4: tombstones and colliding keys on the probe path -------------------------------------------------------------------
def test_carve_through_chains_and_tombstones(gpu_ctx):
    """Four families of keys that share a home slot (chains of 200 to 260 slots, one wrapping the table's end), a third of
    all voxels erased first (tombstones inside the chains), a table at its smallest: every probe of a family voxel walks
    its chain.  Rays run to points behind the family voxels and behind absent keys of the same homes."""
    import test_voxel_table as vt
    sc = vt.Scene()
    for name in ("slot", "wrap", "b"):
        vt.check_chain(sc.fam[name], vt.CRAFT_MASK)
    gpu_ctx.map_reset(vt.VOXEL, 4096)
    gpu_ctx.map_upsert(sc.keys, sc.means, sc.covs)
    assert gpu_ctx.map_size() == (len(sc.keys), vt.CRAFT_SLOTS)
    rng = np.random.default_rng(8)
    gone = rng.random(len(sc.keys)) < 1.0 / 3.0
    gpu_ctx.map_erase(sc.keys[gone])
    left = sc.keys[~gone]
    assert gpu_ctx.map_size() == (len(left), vt.CRAFT_SLOTS)          # no rehash: the tombstones are in the table
    through = np.concatenate([sc.fam["slot"], sc.fam["wrap"], sc.fam["b"], sc.fam["b3"], sc.absent["slot"][:100],
                              sc.ordinary[:500]])
    centres = (through.astype(np.float64) + 0.5) * vt.VOXEL
    inside = (left[::3].astype(np.float64) + rng.uniform(0.1, 0.9, size=(len(left[::3]), 3))) * vt.VOXEL
    pts = np.concatenate([centres * 1.15 + 0.01, inside])
    pts = pts[rng.permutation(len(pts))]
    T = np.eye(4)
    T[:3, 3] = (0.05, -0.04, 0.06)
    p = Params(origin=(0.0, 0.0, 0.0), max_range=80.0, min_hits=1)
    want = mc.carve(left, vt.VOXEL, pts, T, p)
    in_family = mc.match(np.concatenate(list(sc.fam.values())), left[want.removed]) >= 0
    assert want.removed.sum() > 300 and in_family.sum() > 100 and want.shielded > 100
    before = state(gpu_ctx)
    gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
    keys, st = gpu_ctx.map_carve_resident(T, p.as_dict())
    assert same_bits(mc.sorted_keys(keys), mc.sorted_keys(left[want.removed].astype(np.int32)))
    assert counts_of(st) == want.counts()
    assert same_state(state(gpu_ctx), without(before, keys)) and gpu_ctx.map_size() == (len(left) - st.removed, vt.CRAFT_SLOTS)


# ---- 5: the deferred form -----------------------------------------------------------------------------------------------
def frame_poses(T, frames=5):
    out = []
    for f in range(frames):
        P = np.array(T)
        P[:3, 3] += (0.37 * f, -0.21 * f, 0.05 * f)
        out.append(P)
    return out


@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
def test_async_pair_gives_the_sync_pair_and_the_totals(vmap, scene, raw):
    from eskf_lio_amd import capi, synth
    pts, T = scene[0][:2000], scene[1]
    covs = synth.disc_covariances(3, 16, np.arange(len(pts), dtype=np.uint64))
    p = Params(origin=ORIGIN, min_hits=2, margin=VOXEL).as_dict()
    with capi.Context(0) as sync, capi.Context(0) as deferred, capi.Context(0) as plain:
        for c in (sync, deferred, plain):
            if raw:
                c.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
            c.map_reset(VOXEL, len(vmap.keys))
            c.map_insert_scan(vmap.means, vmap.covs, np.eye(4), CAP)
            c.scan_upload(pts, covs)
            assert c.map_carve_totals() == (0, 0)
        rays = removed = 0
        syncs = {}
        for T_f in frame_poses(T):
            _, st = sync.map_carve_resident(T_f, p, keys=False)
            sync.map_insert_resident(T_f, CAP)
            rays, removed = rays + st.rays, removed + st.removed
            for name, c in (("carve", deferred), ("plain", plain)):
                c.frame_stats(reset=True)
                if name == "carve":
                    c.map_carve_resident_async(T_f, p)
                c.map_insert_resident_async(T_f, CAP)
                syncs.setdefault(name, []).append(c.frame_stats().host_syncs)
        # no synchronisation a frame did not have before: the first frame none, every later one the one that settles the
        # insertion of the frame before
        assert syncs["carve"] == syncs["plain"] == [0, 1, 1, 1, 1]
        assert removed > 100 and 4 * len(pts) < rays <= 5 * len(pts)
        assert deferred.map_carve_totals() == sync.map_carve_totals() == (rays, removed)
        assert same_state(state(deferred, raw), state(sync, raw))
        assert deferred.map_size() == sync.map_size() and not same_state(state(plain), state(sync))
        deferred.map_reset(VOXEL, 0)
        assert deferred.map_carve_totals() == (0, 0) and sync.map_carve_totals() == (rays, removed)


def test_async_waits_for_nothing(vmap, scene):
    """Nothing pending: the deferred carve synchronises not at all, and neither does a second one behind it (a pending
    carve makes no deferred call wait); vgicp_map_size then settles both with one synchronisation."""
    from eskf_lio_amd import capi
    pts, T = scene[0][:1000], scene[1]
    p = Params(origin=ORIGIN).as_dict()
    with capi.Context(0) as ctx:
        load(ctx, vmap, 4 * len(vmap.keys))
        ctx.scan_upload(pts, scan_covs(len(pts)))
        want = reference(vmap, pts, T, Params(origin=ORIGIN))
        ctx.frame_stats(reset=True)
        ctx.map_carve_resident_async(T, p)
        assert ctx.frame_stats().host_syncs == 0
        ctx.map_carve_resident_async(T, p)
        ctx.map_insert_resident_async(T, CAP)
        assert ctx.frame_stats().host_syncs == 0 and ctx.frame_stats().kernel_launches >= 6
        ctx.frame_stats(reset=True)
        assert ctx.map_carve_totals() == (2 * want.rays, int(want.removed.sum()))
        assert ctx.frame_stats().host_syncs == 1


def test_a_pending_carve_is_settled_before_the_table_grows(vmap, scene):
    """The deferred insertion behind a deferred carve makes the table grow (the rehash leaves the tombstones behind): the
    carve's count is taken first, and the map is the synchronous pair's."""
    from eskf_lio_amd import capi, synth
    pts, T = scene[0][:1000], scene[1]
    p = Params(origin=ORIGIN).as_dict()
    more = synth.make_map(60_000, voxel_size=VOXEL)
    filler = more.keys[:45_000] + np.array([500, 0, 0], dtype=np.int32)
    sizes = []
    with capi.Context(0) as ctx, capi.Context(0) as twin:
        for c in (ctx, twin):
            c.map_reset(VOXEL, 0)
            c.map_upsert(vmap.keys, vmap.means, vmap.covs)
            c.map_upsert(filler, more.means[:45_000], more.covs[:45_000])
            assert c.map_size() == (65_000, 131_072)          # 1 000 more and the load passes one half
            c.scan_upload(pts, scan_covs(len(pts)))
        ctx.map_carve_resident_async(T, p)
        ctx.map_insert_resident_async(T, CAP)
        _, st = twin.map_carve_resident(T, p, keys=False)
        twin.map_insert_resident(T, CAP)
        assert st.removed > 100
        for c in (ctx, twin):
            sizes.append(c.map_size())
        assert sizes[0] == sizes[1] and sizes[0][1] > 131_072
        assert same_state(state(ctx), state(twin)) and ctx.map_carve_totals() == twin.map_carve_totals() == (st.rays, st.removed)


# ---- 6: refusals --------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order(vmap, scene):
    from eskf_lio_amd import capi
    pts, T = scene[0][:300], scene[1]
    lib = capi.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    good = capi.pose_to_abi(T)
    bad = good.copy()
    bad[13] = np.inf
    keys = np.full((len(vmap.keys), 3), 0x5A5A5A5A, dtype=np.int32)
    stats, removed = capi.CarveStats(), C.c_size_t(77)
    nan, inf = float("nan"), float("inf")

    def sync(ctx, pose=good, with_params=True, **kw):
        C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
        keys[:] = 0x5A5A5A5A
        removed.value = 77
        cp = capi.carve_params(**dict(Params(origin=ORIGIN).as_dict(), **kw))
        return lib.vgicp_map_carve_resident(ctx._h if ctx is not None else None, pose.ctypes.data_as(dp) if pose is not None else None,
                                            C.byref(cp) if with_params else None, len(keys), keys.ctypes.data_as(ip),
                                            C.byref(removed), C.byref(stats))

    def deferred(ctx, pose=good, with_params=True, **kw):
        C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
        keys[:] = 0x5A5A5A5A
        removed.value = 77
        cp = capi.carve_params(**dict(Params(origin=ORIGIN).as_dict(), **kw))
        return lib.vgicp_map_carve_resident_async(ctx._h if ctx is not None else None,
                                                  pose.ctypes.data_as(dp) if pose is not None else None,
                                                  C.byref(cp) if with_params else None)

    def untouched():
        return np.all(keys == 0x5A5A5A5A) and bytes(stats) == b"\xa5" * C.sizeof(stats) and removed.value == 77

    for call in (sync, deferred):
        assert call(None) == capi.ERR_BAD_ARGUMENT and untouched()                                          # 1
        with capi.Context(0) as ctx:
            # 3 in front of everything behind it
            assert call(ctx, pose=None, with_params=False) == capi.ERR_NOT_READY and "map" in ctx.last_error()
            load(ctx, vmap)
            assert call(ctx, pose=None, margin=nan) == capi.ERR_NOT_READY and "scan" in ctx.last_error() and untouched()
            ctx.scan_upload(pts, scan_covs(len(pts)))
            before, generation = state(ctx), ctx.counter(COUNTER_SCAN_GENERATION)

            def refused(text, **kwargs):
                assert call(ctx, **kwargs) == capi.ERR_BAD_ARGUMENT and text in ctx.last_error(), (kwargs, ctx.last_error())
                assert untouched()
                assert same_state(state(ctx), before) and ctx.counter(COUNTER_SCAN_GENERATION) == generation

            refused("NULL pointer", pose=None, margin=nan)                                                   # 4
            refused("NULL pointer", with_params=False, pose=bad)
            refused("not finite", pose=bad, margin=nan)                                                      # 5 before 6
            refused("not finite", origin=(0.0, nan, 0.0), margin=-1.0)
            for margin in (nan, -1.0, -1e-300, inf, -inf):                                                   # 6 before 7
                refused("margin must be", margin=margin, max_range=nan)
            for max_range in (nan, 0.0, -1.0, inf, 4096.5 * VOXEL):                                          # 7 before 8
                refused("max_range must be", max_range=max_range, min_hits=0)
            refused("must be >= 1", min_hits=0)                                                              # 8
            refused("must be >= 1", stride=0)
            # 9: a communicator (one rank is enough) behind 8
            ctx.comm_init(1, 0, ctx.comm_unique_id())
            refused("must be >= 1", stride=0)
            refused("single-device")
            ctx.comm_destroy()
            assert call(ctx, max_range=4096.0 * VOXEL) == capi.OK
            assert not same_state(state(ctx), before)
        with capi.Context([0, 0]) as multi:                                                                  # 9
            assert call(multi) == capi.ERR_NOT_READY                       # 3 before 9: no map
            multi.map_reset(VOXEL, len(vmap.keys))
            multi.map_upsert(vmap.keys, vmap.means, vmap.covs)
            multi.scan_upload(pts, scan_covs(len(pts)))
            before = state(multi)
            assert call(multi, min_hits=0) == capi.ERR_BAD_ARGUMENT and "must be >= 1" in multi.last_error()   # 8 before 9
            assert call(multi) == capi.ERR_BAD_ARGUMENT and "single-device" in multi.last_error() and untouched()
            assert same_state(state(multi), before)
            assert multi.map_carve_totals() == (0, 0)


# ---- 7: the point of it -----------------------------------------------------------------------------------------------
def test_the_point_of_it(oracle):
    """A scene (ground, walls, clutter) plus a box of "ghost" points inserted once; then the scene WITHOUT the box is seen
    from three poses.  Every ghost voxel that the brute-force certain count puts in free space is gone, the scene's
    voxels that hold returns are all still there, and an align from a perturbed guess afterwards matches no point into a
    former ghost voxel."""
    from eskf_lio_amd import capi, synth
    world = synth.make_lidar_scan(12_000, seed=21, extent=25.0)
    world = world[np.linalg.norm(world[:, :2], axis=1) > 1.5]
    rng = np.random.default_rng(2)
    ghost = np.array([4.0, -3.0, 0.6]) + rng.uniform(0.0, 1.0, size=(600, 3)) * (1.5, 1.5, 1.2)
    ghost_keys = np.unique(mc.keys_of(ghost, VOXEL)[0], axis=0)
    scene_keys = np.unique(mc.keys_of(world, VOXEL)[0], axis=0)
    ghost_keys = ghost_keys[mc.match(scene_keys, ghost_keys) < 0]          # voxels that only the ghost fills
    assert len(ghost_keys) >= 20
    poses = [synth.se3_to_SE3(xi) for xi in ((0.0, 0.0, 1.2, 0.0, 0.0, 0.0), (1.0, 0.8, 1.2, 0.0, 0.0, 0.3),
                                             (-0.8, 1.5, 1.3, 0.01, -0.02, -0.4))]
    p = Params(origin=(0.0, 0.0, 0.0), margin=VOXEL, min_hits=3, max_range=40.0)
    covs = synth.disc_covariances(7, 16, np.arange(len(world), dtype=np.uint64))
    with capi.Context(0) as ctx:
        ctx.map_reset(VOXEL, 0)
        ctx.map_insert_scan(world, covs, np.eye(4), CAP)
        ctx.map_insert_scan(ghost, covs[:len(ghost)], np.eye(4), CAP)
        keys0 = ctx.map_export()[0]
        assert np.all(mc.match(keys0, ghost_keys) >= 0)
        must_go = np.zeros(len(ghost_keys), dtype=bool)
        for T in poses:
            scan = synth._apply(synth.invert_pose(T), world)               # the scene as the sensor at T sees it
            certain, _ = mc.slab_counts(ghost_keys, VOXEL, scan, T, p)
            at = mc.match(ghost_keys, mc.keys_of(mc.transform(T, scan), VOXEL)[0])
            shield = np.zeros(len(ghost_keys), dtype=bool)
            shield[at[at >= 0]] = True
            must_go |= (certain >= p.min_hits) & ~shield
            ctx.scan_upload(scan, covs)
            ctx.map_carve_resident(T, p.as_dict(), keys=False)
        assert must_go.sum() >= 0.8 * len(ghost_keys)
        keys1 = ctx.map_export()[0]
        assert np.all(mc.match(keys1, ghost_keys[must_go]) < 0)            # gone
        held = np.unique(mc.keys_of(mc.transform(poses[-1], scan), VOXEL)[0], axis=0)
        assert np.all(mc.match(keys1, held) >= 0)                          # the last scan's own voxels all stay
        rays, removed = ctx.map_carve_totals()
        assert 2.9 * len(world) < rays <= 3 * len(world) and removed >= must_go.sum()    # (a return within the margin casts no ray)
        # an align from a perturbed guess: no correspondence into a former ghost voxel
        T = poses[0]
        ctx.scan_upload(synth._apply(synth.invert_pose(T), np.concatenate([world, ghost])), np.concatenate([covs, covs[:len(ghost)]]))
        guess = T @ synth.se3_to_SE3((0.04, -0.03, 0.02, 0.003, -0.002, 0.004))
        r = ctx.align_resident(guess, 30, 1e-8, 0.999999)
        rep = ctx.points_resident(r.pose, d2=False, sq_error=False, weight=False)
        at = mc.keys_of(mc.transform(r.pose, synth._apply(synth.invert_pose(T), np.concatenate([world, ghost]))), VOXEL)[0]
        matched = (rep.status & capi.POINT_MATCHED) != 0
        assert matched.sum() > 0.5 * len(world)
        assert np.all(mc.match(ghost_keys[must_go], at[matched]) < 0)
        assert not matched[len(world):][mc.match(ghost_keys[must_go], at[len(world):]) >= 0].any()


# ---- 8: the drop-in classes and the replay ------------------------------------------------------------------------------
def test_drop_in_frames_with_carve_end_at_the_abi_chain():
    """CloudPreprocessor::process -> ICP::align -> LocalMap::updateLocalMap through the C++ classes with LocalMap::setCarve:
    every update is vgicp_map_carve_resident_async, then the resident insertion, so poses, map and totals are bit for bit
    those of the bare chain on the C ABI."""
    from eskf_lio_amd import capi, host
    from test_multi_device import _NO_GATE, _frame_inputs
    st, t, ext, raws = _frame_inputs(frames=4, n=20_000)
    carve = dict(margin=0.3, max_range=30.0, min_hits=2, stride=1, origin=tuple(ext[:3, 3]))
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
            c.map_carve_resident_async(pose, carve)
            c.map_insert_resident_async(pose, CAP)
        want_totals = c.map_carve_totals()
        want_state = state(c, True)
    assert want_totals[0] > 0 and want_totals[1] > 0

    pre = host.CloudPreprocessor(0.3, ext, "deferred")
    icp = host.ICP(30, 1e-6, 0.9999)
    lmap = host.LocalMap(0.3, CAP, dict(_NO_GATE, device_resident=True))            # keeps raw points, in the shadow grid
    assert lmap.carveTotals() == (0, 0)
    lmap.setCarve(**carve)
    assert lmap.savesRawPoints()
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
    assert lmap.carveTotals() == want_totals
    keys, means, covs, counts = lmap.export()
    order = np.lexsort(keys.T)
    assert all(same_bits(x, y) for x, y in zip((keys[order], means[order], covs[order], counts[order]), want_state[:4]))
    # switched off again: the next frame carves nothing
    lmap.clearCarve()
    fr = host.Frame(raws[1], t, st)
    fr.run(pre, icp, lmap, pose)
    fr.end()
    assert lmap.carveTotals() == want_totals
    for bad in (dict(max_range=0.0), dict(max_range=30.0, margin=-1.0), dict(max_range=30.0, min_hits=0),
                dict(max_range=30.0, stride=0), dict(max_range=0.3 * 4097)):
        with pytest.raises(ValueError, match="setCarve"):
            lmap.setCarve(**bad)
    # a map that already holds frames cannot move its raw points to the device; a host-authoritative map is never carved
    late = host.LocalMap(0.3, CAP, dict(_NO_GATE, device_resident=True))
    fr = host.Frame(raws[0], t, st)
    fr.run(pre, icp, late, np.eye(4), first_frame=True)
    fr.end()
    with pytest.raises(ValueError):
        late.setCarve(**carve)
    with pytest.raises(ValueError, match="device-resident"):
        host.LocalMap(0.3, CAP).setCarve(**carve)


def test_replay_on_the_resident_chain():
    """local_map.carve on replay.DeviceBackend: voxels are removed, the totals say so, and the map is another than the plain
    chain's; without the key the run is the plain one."""
    from eskf_lio_amd import replay, synth
    from replay_backends import stream_events
    stream = synth.make_sensor_stream(frames=4, points_per_frame=6_000)[0]
    runs = {}
    for name, carve in (("plain", None), ("carve", dict(max_range=30.0, margin=0.3, min_hits=2))):
        cfg = replay.DEFAULT_CONFIG if carve is None else \
            dict(replay.DEFAULT_CONFIG, local_map=dict(replay.DEFAULT_CONFIG["local_map"], carve=carve))
        backend = replay.DeviceBackend(cfg, 0)
        traj = replay.Odometry(cfg, backend).run(stream_events(replay, stream))
        runs[name] = (traj, state(backend.ctx), backend.ctx.map_carve_totals())
        backend.ctx.close()
    assert len(runs["plain"][0]) == 4 and runs["plain"][2] == (0, 0)
    rays, removed = runs["carve"][2]
    assert rays > 0 and removed > 0 and not same_state(runs["carve"][1], runs["plain"][1])
    with pytest.raises(ValueError, match="single-device"):
        replay.DeviceBackend(dict(replay.DEFAULT_CONFIG, local_map=dict(replay.DEFAULT_CONFIG["local_map"], carve=dict(max_range=30.0))), [0, 0])
