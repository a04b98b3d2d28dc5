"""Submap as scan on the device (include/vgicp_hip_map_submap.h): vgicp_scan_from_map and vgicp_scan_from_map_keys.

The content of every from-map scan is compared with == against the numpy restatement of the rule
(tests/map_submap_reference.py, checked on its own by tests/test_map_submap_cpu.py) applied to what the device itself
exports; the order against the table's home slots (tests/test_voxel_table.py's voxel_hash) on keys that do not collide;
the scan as a scan against an upload of its own download; and the point of it all, a piece of one map registered on
another, against the basin condition and the oracle.

No test models which of two keys that collide inside ONE batch wins the home slot (the claims race), so the order check
and the two-context check are made on maps whose keys have distinct home slots: there a key sits at its home."""
import ctypes as C
import math

import numpy as np
import pytest

import map_levels_reference as ml
import map_submap_reference as ms
from conftest import POSE_TOL_M, POSE_TOL_RAD, pose_error
from eskf_lio_amd import capi, synth
from test_voxel_table import next_pow2, voxel_hash

pytestmark = pytest.mark.gpu

VOXEL = 0.5          # centres and the radii below are exact in binary
COUNTER_SCAN_GENERATION = 5
INF = math.inf


def random_keys(n, span, seed):
    """n distinct keys on both sides of zero."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(-span, span, size=(3 * n + 8, 3)), axis=0).astype(np.int32)
    assert len(keys) >= n
    return keys[rng.permutation(len(keys))[:n]]


def payload(keys, seed):
    rng = np.random.default_rng(seed)
    means = (keys.astype(np.float64) + rng.uniform(0.1, 0.9, size=keys.shape)) * VOXEL
    covs = synth.disc_covariances(seed + 1, 16, np.arange(len(keys), dtype=np.uint64))
    return means, covs


def upsert_map(ctx, keys, seed=5, hint=None):
    means, covs = payload(keys, seed)
    ctx.map_reset(VOXEL, len(keys) if hint is None else hint)
    ctx.map_upsert(keys, means, covs)


def counted_map(ctx, keys, seed=7, cap=6):
    """The keys with 1 .. 5 points each through vgicp_map_insert_scan: counts differ."""
    rng = np.random.default_rng(seed)
    per = rng.integers(1, 6, size=len(keys))
    k = np.repeat(keys.astype(np.int64), per, axis=0)
    pts = (k + rng.uniform(0.1, 0.9, size=k.shape)) * VOXEL
    pts = pts[rng.permutation(len(pts))]
    covs = synth.disc_covariances(seed + 1, 16, np.arange(len(pts), dtype=np.uint64))
    ctx.map_reset(VOXEL, len(keys))
    ctx.map_insert_scan(pts, covs, np.eye(4), cap)
    return per


def frame_of(yaw_deg=30.0, pitch_deg=-10.0, t=(1.25, -0.5, 0.75)):
    y, p = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    Rz = np.array([[np.cos(y), -np.sin(y), 0.0], [np.sin(y), np.cos(y), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[np.cos(p), 0.0, np.sin(p)], [0.0, 1.0, 0.0], [-np.sin(p), 0.0, np.cos(p)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry, t
    return T


def delivered(ctx):
    """(keys, points, covs, counts) in scan order."""
    pts, covs = ctx.scan_download()
    keys, counts = ctx.scan_from_map_keys()
    assert len(keys) == len(counts) == len(pts) == len(covs)
    return keys, pts, covs, counts


def assert_is_the_rule(ctx, st, exported, h, center, radius, frame=None, min_count=0, what=""):
    """The resident scan and its keys, sorted by key, against the restatement applied to `exported`, with == on every
    double; the four counts of the stats."""
    want = ms.submap(*exported, h, center, radius, frame, min_count)
    assert (st.voxels, st.points, st.too_far, st.too_few) == (want.voxels, len(want), want.too_far, want.too_few), (what, st)
    if len(want) == 0:
        return want
    k, p, c, n = ms.by_key(*delivered(ctx))
    assert np.array_equal(k, want.keys) and np.array_equal(n, want.counts), what
    assert np.array_equal(p, want.points) and np.array_equal(c, want.covs), what          # ==, NaN-free
    return want


# ---- 1. content at small sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 5000))
def test_the_whole_map_under_the_identity_is_the_export(gpu_ctx, n):
    keys = random_keys(n, 3 if n < 100 else 5 if n < 300 else 12, seed=n)
    assert (keys.min(axis=0) < 0).all() or n == 1
    upsert_map(gpu_ctx, keys)
    st = gpu_ctx.scan_from_map(gpu_ctx, (0.0, 0.0, 0.0), INF)
    assert st.points == n and st.launches == 3 and st.device_seconds > 0.0
    exported = gpu_ctx.map_export()
    assert_is_the_rule(gpu_ctx, st, exported, VOXEL, (0.0, 0.0, 0.0), INF, what=f"n {n}")
    k, p, c, cnt = ms.by_key(*delivered(gpu_ctx))
    ek, em, ec, en = ml.sort_by_key(*exported)
    assert np.array_equal(k, ek) and np.array_equal(cnt, en)
    assert np.array_equal(p, em) and np.array_equal(c, ec)          # the stored means and covariances, ==
    print(f"n {n}: slots {gpu_ctx.map_size()[1]} device {1e6 * st.device_seconds:.1f} us wall {1e6 * st.seconds:.1f} us")


# ---- 2. selection and transform ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", (0, 3))
def test_a_sphere_a_frame_and_a_least_count(gpu_ctx, min_count):
    """Centre (0.25, 0.25, 0.25) is the centre of voxel 0; radius 2.5 = |(3, 4, 0)| voxels: 30 centres lie exactly on it."""
    keys = np.stack(np.meshgrid(*[np.arange(-9, 9)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    keys = keys[np.random.default_rng(2).permutation(len(keys))[:5000]]
    per = counted_map(gpu_ctx, keys)
    center, radius, frame = (0.25, 0.25, 0.25), 2.5, frame_of()
    exported = gpu_ctx.map_export()
    d2 = ((exported[0].astype(np.int64)) ** 2).sum(axis=1)
    assert int((d2 == 25).sum()) >= 10          # on the sphere, and kept
    st = gpu_ctx.scan_from_map(gpu_ctx, center, radius, frame, min_count=min_count)
    want = assert_is_the_rule(gpu_ctx, st, exported, VOXEL, center, radius, frame, min_count, what=f"min_count {min_count}")
    inside = int((d2 <= 25).sum())
    assert st.too_far == len(keys) - inside and st.points + st.too_few == inside
    assert (st.too_few > 0) == (min_count == 3) and len(want) > 50 and len(np.unique(per)) > 2
    on_sphere = exported[0][(d2 == 25) & (exported[3] >= min_count)]
    assert len(on_sphere) and all((want.keys == k).all(axis=1).any() for k in on_sphere)


# ---- 3. placement in the table ------------------------------------------------------------------------------------------
def collision_free(candidates, slots, taken=()):
    """Those of the candidate keys whose home slots are distinct (and not in `taken`), with the homes: such a key sits
    at its home whatever the order of the claims."""
    home = (voxel_hash(candidates) & np.uint32(slots - 1)).astype(np.int64)
    _, first = np.unique(home, return_index=True)
    first = first[~np.isin(home[first], np.asarray(list(taken), dtype=np.int64))]
    return candidates[first], home[first]


def test_only_the_last_workgroup_of_slots_is_selected_and_the_order_is_the_slots(gpu_ctx):
    slots = 4096
    grid = np.stack(np.meshgrid(*[np.arange(-12, 12)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    grid = grid[np.argsort((grid.astype(np.int64) ** 2).sum(axis=1), kind="stable")]          # the near keys choose their homes first
    keys, home = collision_free(grid, slots)
    d2 = (keys.astype(np.int64) ** 2).sum(axis=1)
    near = (d2 <= 36) & (home >= slots - 1024)          # inside the sphere AND at home in the last 1 024 slots
    far = (d2 > 64) & (home < slots - 1024)
    far[np.flatnonzero(far)[600:]] = False
    pick = near | far
    assert near.sum() >= 100 and far.sum() == 600 and (home[near] >= slots - 64).any()
    upsert_map(gpu_ctx, keys[pick], hint=1000)
    assert gpu_ctx.map_size() == (int(pick.sum()), slots)
    st = gpu_ctx.scan_from_map(gpu_ctx, (0.25, 0.25, 0.25), 3.0)
    assert (st.points, st.too_far, st.too_few) == (int(near.sum()), 600, 0)
    got, _ = gpu_ctx.scan_from_map_keys()
    want = keys[near][np.argsort(home[near])]          # ascending slot = ascending home
    assert np.array_equal(got, want)
    # the whole map: still ascending slots
    st = gpu_ctx.scan_from_map(gpu_ctx, (0.0, 0.0, 0.0), INF)
    got, _ = gpu_ctx.scan_from_map_keys()
    assert np.array_equal(got, keys[pick][np.argsort(home[pick])])
    assert (np.diff((voxel_hash(got) & np.uint32(slots - 1)).astype(np.int64)) > 0).all()


def test_nothing_selected_leaves_no_resident_scan(gpu_ctx):
    keys = random_keys(300, 4, seed=9)
    upsert_map(gpu_ctx, keys)
    means, covs = payload(keys[:50], 3)
    gpu_ctx.scan_upload(means, covs)
    assert gpu_ctx.align_resident(np.eye(4), 2, 1e-6, 2.0).status == capi.OK
    generation = gpu_ctx.counter(COUNTER_SCAN_GENERATION)
    st = gpu_ctx.scan_from_map(gpu_ctx, (100.0, 0.0, 0.0), 1.0)
    assert (st.points, st.too_far, st.too_few, st.voxels) == (0, 300, 0, 300)
    assert gpu_ctx.counter(COUNTER_SCAN_GENERATION) == generation + 1
    with pytest.raises(capi.VgicpError) as e:
        gpu_ctx.align_resident(np.eye(4), 2, 1e-6, 2.0)
    assert e.value.code == capi.ERR_NOT_READY
    keys_out, counts_out = gpu_ctx.scan_from_map_keys()
    assert len(keys_out) == len(counts_out) == 0
    # ... and an empty map
    gpu_ctx.map_reset(VOXEL, 0)
    st = gpu_ctx.scan_from_map(gpu_ctx, (0.0, 0.0, 0.0), INF)
    assert (st.points, st.voxels, st.launches) == (0, 0, 0)


# ---- 4. tombstones and growth --------------------------------------------------------------------------------------------
def test_tombstones_never_appear_and_a_rehash_changes_nothing_of_the_content(gpu_ctx):
    keys = random_keys(5000, 12, seed=21)
    upsert_map(gpu_ctx, keys, hint=5000)
    slots0 = gpu_ctx.map_size()[1]
    removed = gpu_ctx.map_evict((0.25, 0.25, 0.25), 5.0)
    erased = gpu_ctx.map_export()[0][::7]
    gpu_ctx.map_erase(erased)
    assert removed > 500 and gpu_ctx.map_size() == (5000 - removed - len(erased), slots0)
    frame = frame_of(-75.0, 20.0)
    st = gpu_ctx.scan_from_map(gpu_ctx, (0.0, 0.0, 0.0), INF, frame)
    want = assert_is_the_rule(gpu_ctx, st, gpu_ctx.map_export(), VOXEL, (0.0, 0.0, 0.0), INF, frame, what="tombstones")
    assert st.voxels == 5000 - removed - len(erased)
    gone = {tuple(k) for k in erased}
    assert not gone & {tuple(k) for k in want.keys}
    assert ((((want.keys.astype(np.float64) + 0.5) * VOXEL - 0.25) ** 2).sum(axis=1)).max() <= 25.0          # what eviction kept
    # growth: enough new voxels to rehash into a larger table, which drops the tombstones
    more = random_keys(20000, 30, seed=22)
    more = more[(np.abs(more) > 12).any(axis=1)]
    means, covs = payload(more, 23)
    gpu_ctx.map_upsert(more, means, covs)
    assert gpu_ctx.map_size()[1] > slots0
    st = gpu_ctx.scan_from_map(gpu_ctx, (1.0, -2.0, 0.5), 9.0, frame, min_count=1)
    want = assert_is_the_rule(gpu_ctx, st, gpu_ctx.map_export(), VOXEL, (1.0, -2.0, 0.5), 9.0, frame, 1, what="grown")
    assert len(want) > 500 and not gone & {tuple(k) for k in want.keys}


# ---- 5. levels --------------------------------------------------------------------------------------------------------------
def test_a_level_is_a_source_like_the_map_and_is_rebuilt_first(gpu_ctx):
    keys = random_keys(5000, 12, seed=31)
    counted_map(gpu_ctx, keys)
    gpu_ctx.map_levels_build(3)
    center, frame = (0.5, 0.5, -0.5), frame_of(12.0, 3.0, (0.0, 2.0, 0.0))
    for level, radius in ((1, 4.0), (3, INF)):
        st = gpu_ctx.scan_from_map(gpu_ctx, center, radius, frame, min_count=4, level=level)
        want = assert_is_the_rule(gpu_ctx, st, gpu_ctx.map_level_export(level), VOXEL * 2 ** level, center, radius, frame, 4,
                                  what=f"level {level}")
        assert st.launches == 3 and len(want) > 10 and st.voxels == gpu_ctx.map_level_size(level)[0]
    # after an insertion, with no rebuild asked for: the level is rebuilt in front of the call
    more = random_keys(700, 16, seed=32)
    means, covs = payload(more, 33)
    gpu_ctx.map_insert_scan(means, covs, np.eye(4), 6)
    st = gpu_ctx.scan_from_map(gpu_ctx, center, INF, frame, level=2)
    assert st.launches == 3 + 2 * 3          # three levels rebuilt, two launches each
    levels = ml.levels_of(*gpu_ctx.map_export(), 2)
    rule = levels[2]
    want = assert_is_the_rule(gpu_ctx, st, (rule.keys, rule.means, rule.covs, rule.counts), VOXEL * 4, center, INF, frame,
                              what="level 2 after an insertion")
    assert len(want) == gpu_ctx.map_level_size(2)[0]
    with pytest.raises(capi.VgicpError) as e:
        gpu_ctx.scan_from_map(gpu_ctx, center, INF, level=4)
    assert e.value.code == capi.ERR_NOT_READY and "vgicp_map_levels_build" in str(e.value)


# ---- 6. determinism ------------------------------------------------------------------------------------------------------
def scan_bytes(ctx):
    keys, pts, covs, counts = delivered(ctx)
    return keys.tobytes() + pts.tobytes() + covs.tobytes() + counts.tobytes()


def collision_free_sequence(ctx):
    """Two batches, an eviction and an erase; every key of the map has a home slot of its own (tombstones included)."""
    slots = next_pow2(4 * 5000)
    grid = np.stack(np.meshgrid(*[np.arange(-14, 14)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    grid = grid[np.random.default_rng(41).permutation(len(grid))]
    keys, home = collision_free(grid, slots)
    first, second = keys[0:8000:2], keys[1:1600:2]
    upsert_map(ctx, first, hint=5000)
    assert ctx.map_size()[1] == slots
    ctx.map_evict((0.25, 0.25, 0.25), 6.0)
    ctx.map_erase(first[::11])
    means, covs = payload(second, 43)
    ctx.map_upsert(second, means, covs)
    assert ctx.map_size()[1] == slots
    return slots


def test_two_calls_and_two_contexts_give_the_same_bytes(gpu_ctx):
    slots = collision_free_sequence(gpu_ctx)
    frame = frame_of()
    gpu_ctx.scan_from_map(gpu_ctx, (0.0, 0.5, 0.0), 5.5, frame)
    one = scan_bytes(gpu_ctx)
    a = gpu_ctx.align_resident(np.eye(4), 5, 1e-6, 2.0, allow_degenerate=True)
    gpu_ctx.scan_from_map(gpu_ctx, (0.0, 0.5, 0.0), 5.5, frame)
    assert scan_bytes(gpu_ctx) == one and len(one) > 100 * 116
    b = gpu_ctx.align_resident(np.eye(4), 5, 1e-6, 2.0, allow_degenerate=True)
    assert np.array_equal(a.pose, b.pose) and np.array_equal(a.normal_eq, b.normal_eq) and np.array_equal(a.corr_count, b.corr_count)
    got, _ = gpu_ctx.scan_from_map_keys()
    assert (np.diff((voxel_hash(got) & np.uint32(slots - 1)).astype(np.int64)) > 0).all()          # ascending slots
    other = capi.Context(0)
    try:
        collision_free_sequence(other)
        other.scan_from_map(other, (0.0, 0.5, 0.0), 5.5, frame)
        assert scan_bytes(other) == one
        c = other.align_resident(np.eye(4), 5, 1e-6, 2.0, allow_degenerate=True)
        assert np.array_equal(a.pose, c.pose) and np.array_equal(a.normal_eq, c.normal_eq)
    finally:
        other.close()


# ---- 7. the scan is a scan -------------------------------------------------------------------------------------------------
def test_an_upload_of_the_download_registers_to_the_same_bits(gpu_ctx):
    keys = random_keys(5000, 12, seed=51)
    upsert_map(gpu_ctx, keys)
    gpu_ctx.map_levels_build(2)
    frame = frame_of(1.0, 0.5, (0.06, -0.04, 0.03))          # rotated: R C R^T is not bitwise symmetric
    gpu_ctx.scan_from_map(gpu_ctx, (0.0, 0.0, 0.0), 6.0, frame)
    pts, covs = gpu_ctx.scan_download()
    assert len(pts) > 1000 and (covs[:, 1] != covs[:, 3]).any()
    third = capi.Context(0)
    try:
        upsert_map(third, keys)
        third.map_levels_build(2)
        third.scan_upload(pts, covs)
        fine = dict(max_iteration=30, translation_sq_threshold=1e-6, cosine_threshold=0.9999)
        for ctx_a, ctx_b in ((gpu_ctx, third),):
            a = ctx_a.align_resident(np.eye(4), **fine)
            b = ctx_b.align_resident(np.eye(4), **fine)
            assert a.iterations == b.iterations >= 1 and np.array_equal(a.pose, b.pose)
            assert np.array_equal(a.corr_count, b.corr_count) and np.array_equal(a.normal_eq, b.normal_eq)
            ea, eb = ctx_a.evaluate_resident([np.eye(4), a.pose]), ctx_b.evaluate_resident([np.eye(4), a.pose])
            for x, y in zip(ea, eb):
                assert (x.correspondences, x.cost, x.sq_error) == (y.correspondences, y.cost, y.sq_error) and x.correspondences > 500
                assert np.array_equal(x.normal_eq, y.normal_eq)
            pa, sa = ctx_a.align_resident_levels(np.eye(4), (2, 1, 0), fine)
            pb, sb = ctx_b.align_resident_levels(np.eye(4), (2, 1, 0), fine)
            assert np.array_equal(pa, pb) and [s.iterations for s in sa] == [s.iterations for s in sb]
            assert all(np.array_equal(x.corr_count, y.corr_count) for x, y in zip(sa, sb))
    finally:
        third.close()


# ---- 8. src == dst and src != dst ------------------------------------------------------------------------------------------
def map_bytes(ctx):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in ctx.map_export())


def test_the_source_is_only_read_and_the_destinations_map_is_not_touched(gpu_ctx):
    src, dst = gpu_ctx, capi.Context(0)
    try:
        keys = random_keys(3000, 10, seed=61)
        counted_map(src, keys)
        upsert_map(dst, random_keys(400, 5, seed=62))
        means, covs = payload(keys[:200], 63)
        src.scan_upload(means, covs)
        src_map, dst_map = map_bytes(src), map_bytes(dst)
        src_scan, src_generation = src.scan_download(), src.counter(COUNTER_SCAN_GENERATION)
        dst_generation = dst.counter(COUNTER_SCAN_GENERATION)
        frame = frame_of()
        st = dst.scan_from_map(src, (0.25, 0.25, 0.25), 3.5, frame, min_count=2)
        assert_is_the_rule(dst, st, src.map_export(), VOXEL, (0.25, 0.25, 0.25), 3.5, frame, 2, what="src != dst")
        assert st.points > 100 and dst.counter(COUNTER_SCAN_GENERATION) == dst_generation + 1
        assert map_bytes(src) == src_map and map_bytes(dst) == dst_map
        assert src.counter(COUNTER_SCAN_GENERATION) == src_generation
        again = src.scan_download()
        assert again[0].tobytes() == src_scan[0].tobytes() and again[1].tobytes() == src_scan[1].tobytes()
        with pytest.raises(capi.VgicpError) as e:          # the source's scan is not one a from-map call made
            src.scan_from_map_keys()
        assert e.value.code == capi.ERR_NOT_READY
        # src == dst: the map is read, the scan replaced
        st = src.scan_from_map(src, (0.25, 0.25, 0.25), 3.5, frame, min_count=2)
        assert map_bytes(src) == src_map and src.counter(COUNTER_SCAN_GENERATION) == src_generation + 1
        assert scan_bytes(src) == scan_bytes(dst)
        # the keys go with the scan: an upload ends them, a capacity below n copies nothing
        w = C.c_size_t(0)
        small = np.full((5, 3), 7, dtype=np.int32)
        rc = capi.load_library().vgicp_scan_from_map_keys(dst._h, 5, small.ctypes.data_as(C.POINTER(C.c_int32)), None, C.byref(w))
        assert rc == capi.ERR_BAD_ARGUMENT and w.value == st.points and (small == 7).all()
        dst.scan_upload(means, covs)
        with pytest.raises(capi.VgicpError) as e:
            dst.scan_from_map_keys()
        assert e.value.code == capi.ERR_NOT_READY
    finally:
        dst.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_come_in_the_headers_order_and_change_nothing(gpu_ctx):
    lib = capi.load_library()
    keys = random_keys(500, 5, seed=71)
    upsert_map(gpu_ctx, keys)
    means, covs = payload(keys[:100], 72)
    gpu_ctx.scan_upload(means, covs)
    empty = capi.Context(0)          # no map
    multi = capi.Context([0, 0])
    try:
        before = (gpu_ctx.counter(COUNTER_SCAN_GENERATION), scan := gpu_ctx.scan_download(), map_bytes(gpu_ctx))

        def call(dst, src, center=(0.0, 0.0, 0.0), radius=1.0, frame=None, level=0, reserved=0):
            p = capi.SubmapParams((C.c_double * 3)(*center), radius, (C.c_double * 16)(*capi.pose_to_abi(np.eye(4) if frame is None else frame)),
                                  0, level, reserved)
            st = capi.SubmapStats()
            C.memset(C.byref(st), 0xA5, C.sizeof(st))
            rc = lib.vgicp_scan_from_map(dst._h if dst else None, src._h if src else None, C.byref(p), C.byref(st))
            assert rc == capi.OK or bytes(st) == b"\xa5" * C.sizeof(st)          # a refused call writes no stats
            return rc, (dst.last_error() if dst else "")

        nan_frame = np.eye(4)
        nan_frame[1, 3] = np.nan
        nan = float("nan")
        cases = (  # every case breaks the rule named and every later one it can
            (3, (multi, gpu_ctx, dict(reserved=1, level=9)), capi.ERR_BAD_ARGUMENT, "multi-device contexts, communicators and peer-connected"),
            (3, (gpu_ctx, multi, dict(reserved=1)), capi.ERR_BAD_ARGUMENT, "vgicp_scan_from_map is not available"),
            (5, (gpu_ctx, empty, dict(reserved=1, level=9, radius=nan)), capi.ERR_BAD_ARGUMENT, "reserved must be 0"),
            (6, (gpu_ctx, empty, dict(level=5, radius=-1.0, center=(nan, 0.0, 0.0))), capi.ERR_BAD_ARGUMENT, "level must be 0 .. VGICP_LEVELS_MAX"),
            (6, (gpu_ctx, gpu_ctx, dict(level=-1)), capi.ERR_BAD_ARGUMENT, "level must be"),
            (7, (gpu_ctx, empty, dict(level=2, radius=nan, frame=nan_frame)), capi.ERR_NOT_READY, "call vgicp_map_levels_build first"),
            (8, (gpu_ctx, empty, dict(center=(0.0, math.inf, 0.0), radius=-1.0)), capi.ERR_BAD_ARGUMENT, "center or frame is not finite"),
            (8, (gpu_ctx, empty, dict(frame=nan_frame, radius=nan)), capi.ERR_BAD_ARGUMENT, "center or frame is not finite"),
            (9, (gpu_ctx, empty, dict(radius=nan)), capi.ERR_BAD_ARGUMENT, "radius must be >= 0"),
            (9, (gpu_ctx, empty, dict(radius=-0.5)), capi.ERR_BAD_ARGUMENT, "radius must be >= 0"),
            (9, (gpu_ctx, empty, dict(radius=-math.inf)), capi.ERR_BAD_ARGUMENT, "radius must be >= 0"),
            (10, (gpu_ctx, empty, dict()), capi.ERR_NOT_READY, "no voxel map"),
        )
        for rule, (dst, src, kw), status, text in cases:
            rc, err = call(dst, src, **kw)
            assert rc == status and text in err, (rule, rc, err)
        # rule 1: no context to leave a text in but dst's own
        assert call(None, gpu_ctx)[0] == call(gpu_ctx, None)[0] == capi.ERR_BAD_ARGUMENT
        assert lib.vgicp_scan_from_map(gpu_ctx._h, gpu_ctx._h, None, None) == capi.ERR_BAD_ARGUMENT
        assert "NULL pointer" in gpu_ctx.last_error()
        after = (gpu_ctx.counter(COUNTER_SCAN_GENERATION), gpu_ctx.scan_download(), map_bytes(gpu_ctx))
        assert after[0] == before[0] and after[2] == before[2]
        assert after[1][0].tobytes() == scan[0].tobytes() and after[1][1].tobytes() == scan[1].tobytes()
        assert gpu_ctx.align_resident(np.eye(4), 2, 1e-6, 2.0).status == capi.OK          # the uploaded scan is still the resident one
        # a radius of 0 and of +infinity are not refused
        assert call(gpu_ctx, gpu_ctx, radius=0.0)[0] == capi.OK
    finally:
        empty.close()
        multi.close()


# ---- 10. the purpose, end to end --------------------------------------------------------------------------------------------
def test_a_piece_of_one_session_registers_on_the_other(gpu_ctx, oracle):
    """ICP::alignSubmap's recipe through capi: B's voxels within 15 m of the anchor with at least two points, in the
    anchor's frame, registered on A from the guess "B's frame is A's" (the anchor itself).  The error is the anchor's
    position against where D puts it.  The basin condition: below half a voxel and below the guess's own 0.198 m.
    Measured on the CPU oracle: 9.4 mm after 8 rounds."""
    a_frames, b_frames, D, anchor = ms.two_sessions(oracle)
    target, source = gpu_ctx, capi.Context(0)
    try:
        target.map_reset(ms.VOXEL, 10000)
        for p, c, pose in a_frames:
            target.map_insert_scan(p, c, pose, ms.CAP)
        source.map_reset(ms.VOXEL, 10000)
        for p, c, pose in b_frames:
            source.map_insert_scan(p, c, pose, ms.CAP)
        st = target.scan_from_map(source, anchor[:3, 3], ms.RADIUS, synth.invert_pose(anchor), min_count=ms.MIN_COUNT)
        assert st.points > 1000
        got = target.align_resident(anchor, **ms.ALIGN)
        error, guess_error = ms.anchor_error(got.pose, D, anchor), ms.anchor_error(anchor, D, anchor)
        print(f"submap of {st.points} points: {got.iterations} rounds, anchor error {1e3 * error:.2f} mm from a guess {1e3 * guess_error:.1f} mm off; "
              f"from-map call {1e6 * st.device_seconds:.1f} us on the device, {1e6 * st.seconds:.1f} us wall")
        assert error < ms.VOXEL / 2 and error < guess_error
        # the oracle's align of the downloaded scan against map A
        omap = oracle.OracleMap(ms.VOXEL, ms.CAP)
        for p, c, pose in a_frames:
            omap.insert(*oracle.transform(p, c, pose))
        pts, covs = target.scan_download()
        ref = omap.align(pts, covs, anchor, ms.ALIGN["max_iteration"], ms.ALIGN["translation_sq_threshold"], ms.ALIGN["cosine_threshold"])
        dt, dr = pose_error(got.pose, ref.pose)
        assert dt < POSE_TOL_M and dr < POSE_TOL_RAD
    finally:
        source.close()
