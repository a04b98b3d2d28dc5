"""The map checkpoint (include/vgicp_hip_map_checkpoint.h) on the device: what the packed blob holds against the map's own
readers and the numpy restatement (tests/map_checkpoint_reference.py), the round trip into a fresh and into a used
context, a session that is stopped and resumed in the middle of a walk of every map update (tests/map_walk_reference.py)
and of a frame chain, and the refusals.  Everything is compared bit for bit.  Only blobs that the host check rejects are
offered as bad ones: the index rules (10 - 14) are exercised on the CPU alone (tests/test_map_checkpoint_cpu.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import map_checkpoint_reference as mc
import map_walk_reference as mw
from conftest import TIGHT_POSE_TOL, pose_error
from eskf_lio_amd import capi, synth
from test_align_batch import assert_same_bits
from test_map_raw_points import grouped
from test_map_submap import COUNTER_SCAN_GENERATION, VOXEL, collision_free, counted_map, random_keys, upsert_map

pytestmark = pytest.mark.gpu

CAP = 6
ALIGN = (12, 1e-6, 0.9999)
LOCATE_WINDOW = (1, 1, 1)
RAYS = dict(margin=0.25, beyond=1.0, max_range=40.0, stride=1)


def build(ctx, n, raw, erased, seed=3):
    """counted_map of n random keys (1 .. 5 points each under cap 6) with or without the raw store, a third of the keys
    erased or none.  -> (keys that stay, tombstones)."""
    keys = random_keys(n, 24, seed)
    ctx.map_reset(VOXEL, 0)          # empties the map: the option is accepted
    ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1 if raw else 0)
    counted_map(ctx, keys, cap=CAP)
    victims = keys[::3] if erased else keys[:0]
    if len(victims):
        ctx.map_erase(victims)
    stay = np.ones(len(keys), dtype=bool)
    stay[::3] = not erased
    return keys[stay], len(victims)


def by_key(keys, *arrays):
    order = np.lexsort(np.asarray(keys).T)
    return (np.asarray(keys)[order],) + tuple(np.asarray(a)[order] for a in arrays)


def scan_for(keys, seed=11, m=400):
    """A scan near the map: the centres of some of its voxels, moved a little."""
    rng = np.random.default_rng(seed)
    pick = keys[rng.permutation(len(keys))[:min(m, len(keys))]]
    pts = (pick + 0.5) * VOXEL + rng.normal(scale=0.02, size=pick.shape)
    return np.ascontiguousarray(pts), synth.disc_covariances(seed + 1, 16, np.arange(len(pts), dtype=np.uint64))


def whole_map_scan(ctx):
    """The whole map as the resident scan, downloaded: (keys, counts, points, covs) in scan order = ascending slot."""
    ctx.scan_from_map(ctx, (0.0, 0.0, 0.0), math.inf)
    keys, counts = ctx.scan_from_map_keys()
    pts, covs = ctx.scan_download()
    return keys, counts, pts, covs


# ---- 1. content ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("erased", [False, True], ids=["whole", "tombstones"])
@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 5000))
def test_the_blob_is_the_map(gpu_ctx, n, raw, erased):
    ctx = gpu_ctx
    keys, tombstones = build(ctx, n, raw, erased)
    blob = ctx.map_checkpoint()
    st = ctx.last_checkpoint
    assert mc.check(blob) == 0 and capi.map_checkpoint_info(blob)["rule"] == 0
    b = mc.parse(blob)
    h = b.header
    voxels, slots = ctx.map_size()
    points = ctx.map_points_size()[0] if raw else 0
    assert (h["voxel_size"], h["slots"], h["voxels"], h["tombstones"], h["raw_points"], h["flags"]) == \
        (VOXEL, slots, voxels, tombstones, points, int(raw)), h
    assert voxels == len(keys) and len(blob) == h["total_bytes"] == 128 + mc.pad8(4 * voxels) + mc.pad8(4 * tombstones) + 128 * voxels + 24 * points
    assert h["checksum"] == mc.checksum(blob[128:].tobytes())
    assert (st.bytes, st.voxels, st.tombstones, st.raw_points) == (len(blob), voxels, tombstones, points)
    assert st.launches == (0 if voxels + tombstones == 0 else 4 if raw and voxels else 3), st
    # the records, sorted by key, are the export; verbatim otherwise
    r = b.records
    assert (r["state"] == 1).all() and (r["spare"] == 0).all()
    got = by_key(r["key"], r["mean"], r["cov"], r["count"])
    for g, w in zip(got, ctx.map_export()):
        assert np.array_equal(g, w)
    # the record order is ascending slot: the order of a from-map scan of the whole map
    if voxels:
        sk, sn, sp, sc = whole_map_scan(ctx)
        assert np.array_equal(r["key"], sk) and np.array_equal(r["count"], sn)
        assert np.array_equal(r["mean"], sp) and np.array_equal(r["cov"], sc)
    assert (np.diff(b.full_slots.astype(np.int64)) > 0).all() and (np.diff(b.tomb_slots.astype(np.int64)) > 0).all()
    assert len(np.intersect1d(b.full_slots, b.tomb_slots)) == 0 and (b.full_slots < slots).all() and (b.tomb_slots < slots).all()
    # per key the raw section is the raw export
    if raw:
        want = grouped(*ctx.map_points_export())
        lists = b.raw_of_record()
        assert len(want) == voxels
        for key, pts in zip(r["key"], lists):
            assert np.array_equal(pts, want[tuple(key.tolist())]), key
    # canonical: a second checkpoint is the same bytes, and the first changed nothing
    assert np.array_equal(ctx.map_checkpoint(), blob)


def test_keys_with_distinct_homes_sit_at_their_homes(gpu_ctx):
    slots = 4096
    grid = np.stack(np.meshgrid(*[np.arange(-10, 10)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    keys, home = collision_free(grid, slots)
    keys, home = keys[:900], home[:900]
    upsert_map(gpu_ctx, keys, hint=1000)
    assert gpu_ctx.map_size() == (900, slots)
    b = mc.parse(gpu_ctx.map_checkpoint())
    order = np.argsort(home)
    assert np.array_equal(b.full_slots, home[order]) and np.array_equal(b.records["key"], keys[order])
    # with tombstones: an erased key's home is in tomb_slots
    gpu_ctx.map_erase(keys[:100])
    b = mc.parse(gpu_ctx.map_checkpoint())
    assert np.array_equal(b.tomb_slots, np.sort(home[:100])) and np.array_equal(b.full_slots, np.sort(home[100:]))


def test_an_empty_map_no_map_and_a_capacity_one_byte_short(gpu_ctx):
    ctx, lib = gpu_ctx, capi.load_library()
    w, st = C.c_size_t(7), capi.CheckpointStats()
    buf = np.full(4096, 0x5A, dtype=np.uint8)
    assert lib.vgicp_map_checkpoint(ctx._h, buf.size, buf.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(st)) == capi.ERR_NOT_READY
    assert lib.vgicp_map_checkpoint_size(ctx._h, C.byref(w)) == capi.ERR_NOT_READY and "vgicp_map_reset" in ctx.last_error()
    assert (buf == 0x5A).all()
    ctx.map_reset(VOXEL, 100)
    blob = ctx.map_checkpoint()
    assert len(blob) == 128 and mc.check(blob) == 0 and ctx.last_checkpoint.launches == 0
    assert mc.parse(blob).header["slots"] == 1024 and np.array_equal(blob[80:], np.zeros(48, dtype=np.uint8))
    for raw in (False, True):
        build(ctx, 300, raw, True)
        size = ctx.map_checkpoint_size()
        buf[:] = 0x5A
        big = np.full(size, 0x5A, dtype=np.uint8)
        w.value = 0
        rc = lib.vgicp_map_checkpoint(ctx._h, size - 1, big.ctypes.data_as(C.c_void_p), C.byref(w), None)
        assert rc == capi.ERR_BAD_ARGUMENT and w.value == size and "capacity" in ctx.last_error() and (big == 0x5A).all()
        assert lib.vgicp_map_checkpoint(ctx._h, size, big.ctypes.data_as(C.c_void_p), C.byref(w), None) == capi.OK and w.value == size
        assert np.array_equal(big, ctx.map_checkpoint())


# ---- 2. the round trip ------------------------------------------------------------------------------------------------------
def readers(ctx, scan):
    """Everything the round trip compares, of a context whose map is built: the slot-order-dependent readers included."""
    out = {}
    out["size"] = ctx.map_size()
    out["export"] = ctx.map_export()
    out["levels"] = ctx.map_levels_build(3).voxels[:4]
    for l in (1, 2, 3):
        out[f"level {l}"] = ctx.map_level_export(l)
    k, n, p, c = whole_map_scan(ctx)
    out["from map"] = (k.tobytes(), n.tobytes(), p.tobytes(), c.tobytes())
    ctx.scan_upload(*scan)
    guess = synth.se3_to_SE3([0.03, -0.02, 0.01, 0.002, -0.001, 0.003])
    out["align"] = ctx.align_resident(guess, *ALIGN, allow_degenerate=True)
    loc = ctx.locate_resident(np.eye(4), 0, LOCATE_WINDOW)
    out["locate"] = (loc.hits.tobytes(), [{k: v for k, v in b.items() if k != "pose"} for b in loc.best])
    out["rays"] = ctx.rays_resident(np.eye(4), RAYS, per_point=False).counts
    return out


def assert_same_readers(got, want):
    assert got["size"] == want["size"] and list(got["levels"]) == list(want["levels"])
    for name in ("export", "level 1", "level 2", "level 3"):
        for g, w in zip(got[name], want[name]):
            assert np.array_equal(g, w), name
    assert got["from map"] == want["from map"] and got["locate"] == want["locate"] and got["rays"] == want["rays"]
    assert_same_bits(got["align"], want["align"], "the restored map against the original")


@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
def test_a_restored_map_is_the_map_slot_for_slot(gpu_ctx, raw):
    a = gpu_ctx
    keys, _ = build(a, 3000, raw, True)
    scan = scan_for(keys)
    blob = a.map_checkpoint()
    raw_lists = grouped(*a.map_points_export()) if raw else None
    want = readers(a, scan)
    assert np.array_equal(a.map_checkpoint(), blob)          # levels and readers do not change the checkpoint
    # into a fresh context, and into one whose map was reset and filled with something else — of the other raw setting
    with capi.Context(0) as fresh, capi.Context(0) as used:
        other, _ = build(used, 500, not raw, False, seed=9)
        used.map_levels_build(2)
        used.scan_upload(*scan_for(other, seed=4))
        generation = used.counter(COUNTER_SCAN_GENERATION)
        held = used.scan_download()
        for ctx in (fresh, used):
            st = ctx.map_restore(blob)
            assert (st.bytes, st.voxels, st.raw_points) == (len(blob), len(keys), a.last_checkpoint.raw_points)
            assert st.launches == (5 if raw else 2), st          # the clear, SCATTER, and the log's three
            assert np.array_equal(ctx.map_checkpoint(), blob)
        # the resident scan of the used context and its generation are untouched
        assert used.counter(COUNTER_SCAN_GENERATION) == generation
        for g, w in zip(used.scan_download(), held):
            assert np.array_equal(g, w)
        for ctx in (fresh, used):
            if raw:
                lists = grouped(*ctx.map_points_export())
                assert set(lists) == set(raw_lists) and all(np.array_equal(lists[k], raw_lists[k]) for k in lists)
            else:
                with pytest.raises(capi.VgicpError):
                    ctx.map_points_size()          # the restore switched the store off with the blob's flag
            assert_same_readers(readers(ctx, scan), want)
            assert np.array_equal(ctx.map_checkpoint(), blob)
    # ... and into the context that made the checkpoint, after its map was reset and filled with something else
    build(a, 500, not raw, False, seed=9)
    assert not np.array_equal(a.map_checkpoint(), blob)
    a.map_restore(blob)
    assert np.array_equal(a.map_checkpoint(), blob)
    if raw:
        lists = grouped(*a.map_points_export())
        assert set(lists) == set(raw_lists) and all(np.array_equal(lists[k], raw_lists[k]) for k in lists)
    assert_same_readers(readers(a, scan), want)
    assert np.array_equal(a.map_checkpoint(), blob)


def test_the_next_growth_is_the_one_the_original_would_have_made(gpu_ctx):
    """The table's size and its tombstones come back, so the insertion that makes the original grow makes the copy grow,
    to the same size."""
    a = gpu_ctx
    keys, tombstones = build(a, 400, False, True)          # 266 voxels and 134 tombstones in 8 192 slots
    blob = a.map_checkpoint()
    assert a.map_size() == (266, 8192) and tombstones == 134
    # 3 750 points: 2 (266 + 134 + 3 750) > 8 192 >= 2 (266 + 3 750) — it is the tombstones that make the table grow
    more = random_keys(3750, 60, 21)
    pts = (more + 0.5) * VOXEL
    covs = synth.disc_covariances(5, 16, np.arange(len(pts), dtype=np.uint64))
    with capi.Context(0) as b:
        b.map_restore(blob)
        sizes = []
        for ctx in (a, b):
            before = ctx.map_size()
            ctx.map_insert_scan(pts, covs, np.eye(4), CAP)
            sizes.append((before, ctx.map_size()))
        assert sizes[0] == sizes[1] and sizes[0][1][1] > sizes[0][0][1], sizes
        for g, w in zip(b.map_export(), a.map_export()):
            assert np.array_equal(g, w)
        assert mc.parse(b.map_checkpoint()).header["tombstones"] == mc.parse(a.map_checkpoint()).header["tombstones"] == 0


# ---- 3. it goes on as if nothing had happened -------------------------------------------------------------------------------
def resumed_walk(oracle, seed, raw, cut):
    """run_walk with the context checkpointed and closed after operation `cut`, a fresh one restored, the model's scan
    uploaded again and the levels asked for again; the rest of the walk runs on the new context against the same model."""
    ops = mw.walk(seed, raw)
    scene, model = mw.Scene(oracle, seed), mw.Model(oracle, mw.CAPS[seed % len(mw.CAPS)])
    ctx, twin = capi.Context(0), capi.Context(0)
    if raw:
        ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
    device = mw.Device(capi, ctx, twin, pose_error, assert_same_bits, TIGHT_POSE_TOL)
    base = [0, 0, 0, 0]          # the totals at the cut: they are the context's, not the map's
    checks = [0]

    def checked(what, fn):
        checks[0] += 1
        try:
            fn()
        except Exception as e:
            raise AssertionError(f"walk seed {seed} raw {raw} cut {cut}: check {checks[0]} ({what}) failed: {e}") from e

    def read(name):
        if name == "totals":
            want = (model.gated_points - base[0], model.gated_refused - base[1]), (model.carve_rays - base[2], model.carve_removed - base[3])
            checked(name, lambda: mw._equal((device.ctx.map_gated_totals(), device.ctx.map_carve_totals()), want, "totals since the cut"))
        else:
            mw.reader(name, model, device, checked)
        model.note_reader(name)

    try:
        for i, op in enumerate(ops):
            model.begin(op.kind)
            mw.apply(op, model, scene, device, checked)
            if op.kind == "reset":
                base[:] = [0, 0, 0, 0]
            if op.kind.startswith("read_"):
                read(op.kind[5:])
            if (i + 1) % mw.FULL_CHECK_EVERY == 0 or i + 1 == len(ops):
                for name in mw.READERS:
                    if name != "points" or raw:
                        read(name)
            if i == cut:
                blob = device.ctx.map_checkpoint()          # settles what is pending, as every reader does
                model.note_reader("checkpoint")
                h = mc.parse(blob).header
                checked("the checkpoint's header", lambda: mw._equal((h["voxels"], h["slots"], h["tombstones"], h["flags"]),
                                                                      (model.voxels, model.slots, model.tombstones, int(raw)), "header"))
                base[:] = [model.gated_points, model.gated_refused, model.carve_rays, model.carve_removed]
                device.ctx.close()
                device.ctx = capi.Context(0)          # the store is off here: the restore switches it
                device.ctx.map_restore(blob)
                device.ctx.scan_upload(model.scan.points, model.scan.covs)
                if model.levels:
                    device.ctx.map_levels_build(model.levels)
                for name in mw.READERS:
                    if name != "points" or raw:
                        read(name)
        return model, ops, checks[0]
    finally:
        device.ctx.close()
        twin.close()


@pytest.mark.parametrize("seed,raw", [(mw.SEEDS[0], True), (mw.SEEDS[1], False)], ids=["raw", "plain"])
def test_a_walk_goes_on_after_a_restore(oracle, seed, raw):
    model, ops, checks = resumed_walk(oracle, seed, raw, mw.WALK_LENGTH // 2)
    assert model.voxels > 0 and checks > 40


@pytest.mark.parametrize("seed,raw", [(mw.SEEDS[0], True), (mw.SEEDS[1], False)], ids=["raw", "plain"])
def test_a_checkpoint_right_after_a_deferred_update_settles_it(oracle, seed, raw):
    ops = mw.walk(seed, raw)
    cuts = [i for i, op in enumerate(ops) if op.kind in mw.DEFERRED and 8 <= i < mw.WALK_LENGTH - 8]
    assert cuts, [op.kind for op in ops]
    model, _, checks = resumed_walk(oracle, seed, raw, cuts[len(cuts) // 2])
    assert model.voxels > 0 and checks > 40


def test_a_frame_chain_goes_on_after_a_restore():
    """2 K frames on A; K on B, checkpoint, restore into C, K more on C: the poses are A's bit for bit, the maps equal."""
    K, cap, h, knn = 4, 20, 0.5, 30
    world = synth.make_lidar_scan(700, seed=0x46524D, extent=12.0)
    truth = [synth.se3_to_SE3([0.05 * f, 0.02 * f, 0.0, 0.0, 0.0, 0.004 * f]) for f in range(2 * K + 1)]
    rng = np.random.default_rng(12)
    sweeps = []
    for T in truth:
        Tinv = synth.invert_pose(T)
        pts = world + rng.normal(scale=0.005, size=world.shape)
        sweeps.append(np.ascontiguousarray(pts @ Tinv[:3, :3].T + Tinv[:3, 3]))

    def first(ctx):
        ctx.map_reset(h, 0)
        ctx.scan_prepare(sweeps[0], None, None, None, 0.25, knn)
        ctx.map_insert_resident_async(np.eye(4), cap)
        return np.eye(4)

    def frames(ctx, pose, lo, hi):
        out = []
        for f in range(lo, hi):
            ctx.scan_prepare(sweeps[f], None, None, None, 0.25, knn)
            r = ctx.align_resident(pose, 30, 1e-6, 0.9999)
            pose = r.pose
            ctx.map_insert_resident_async(pose, cap)          # deferred: the checkpoint is what settles the K-th
            out.append(r)
        return pose, out

    with capi.Context(0) as a, capi.Context(0) as b, capi.Context(0) as c:
        _, want = frames(a, first(a), 1, 2 * K + 1)
        pose, got = frames(b, first(b), 1, K + 1)
        blob = b.map_checkpoint()
        c.map_restore(blob)
        _, rest = frames(c, pose, K + 1, 2 * K + 1)
        for f, (g, w) in enumerate(zip(got + rest, want)):
            assert_same_bits(g, w, f"frame {f + 1}")
        assert a.map_size() == c.map_size()
        for g, w in zip(c.map_export(), a.map_export()):
            assert np.array_equal(g, w)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_rule_and_change_nothing(gpu_ctx):
    ctx, lib = gpu_ctx, capi.load_library()
    build(ctx, 300, True, True)
    blob = ctx.map_checkpoint()
    good = blob.tobytes()
    st = capi.CheckpointStats()
    flipped = bytearray(good)
    flipped[128 + 200] ^= 0x10
    for bad, rule in ((good[:len(good) - 8], 8), (good[:127], 1), (b"VGICPMAX" + good[8:], 1), (bytes(flipped), 9)):
        assert mc.check(bad) == rule          # the host check rejects it: the device never sees it
        rc = lib.vgicp_map_restore(ctx._h, bad, len(bad), C.byref(st))
        assert rc == capi.ERR_BAD_ARGUMENT and f"rule {rule}:" in ctx.last_error(), (rule, ctx.last_error())
        assert np.array_equal(ctx.map_checkpoint(), blob)
    assert lib.vgicp_map_restore(ctx._h, None, 128, None) == capi.ERR_BAD_ARGUMENT and "NULL" in ctx.last_error()
    assert lib.vgicp_map_restore(None, good, len(good), None) == capi.ERR_BAD_ARGUMENT
    w = C.c_size_t(5)
    assert lib.vgicp_map_checkpoint(ctx._h, len(good), None, C.byref(w), None) == capi.ERR_BAD_ARGUMENT and w.value == 5
    assert np.array_equal(ctx.map_checkpoint(), blob)
    # a multi-device context is refused by all three, whatever the blob
    with capi.Context([0, 0]) as multi:
        multi.map_reset(VOXEL, 100)
        buf = np.zeros(len(good), dtype=np.uint8)
        for rc in (lib.vgicp_map_restore(multi._h, good, len(good), None), lib.vgicp_map_checkpoint_size(multi._h, C.byref(w)),
                   lib.vgicp_map_checkpoint(multi._h, buf.size, buf.ctypes.data_as(C.c_void_p), C.byref(w), None)):
            assert rc == capi.ERR_BAD_ARGUMENT and "single-device" in multi.last_error()
        assert multi.map_size()[0] == 0 and not buf.any()
    assert np.array_equal(ctx.map_checkpoint(), blob)
