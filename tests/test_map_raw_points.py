"""The raw points of the device map (VGICP_OPTION_MAP_RAW_POINTS, include/vgicp_hip_map_points.h) against a numpy
restatement of the reference's rule: Voxel::points holds the first maxNumPoints world points that reached the voxel, in
insertion order (include/ESKF_LIO/LocalMap.hpp:63-87, src/LocalMap.cpp:47-58); an evicted or erased voxel loses them, and
a point that later falls into it starts a fresh list.  World points come from the oracle's Transform, keys from its
getVoxelIndex; every comparison is `==`.

All three insertion paths: vgicp_map_insert_scan (sorted segments), vgicp_map_insert_resident on a prepared scan (the
per-voxel lists), vgicp_map_insert_resident_async (settled by the export); growth of the store and rehashes of the table
from a zero capacity hint; the multi-device context; the drop-in classes' save() with the deferred host copy; and the
resident frame chain's one synchronisation per frame with the store on."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VOXEL = 0.8      # map voxel: (ceil(0.8 / 0.3) + 1)^3 = 64 -> a prepared scan goes through the per-voxel lists
PREP_VOXEL = 0.3


# ---- the restatement ------------------------------------------------------------------------------------------------
class RawMap:
    """LocalMap's voxel grid with Voxel::points only: key -> the first `cap` world points, in insertion order."""

    def __init__(self, oracle, voxel_size):
        self.oracle, self.voxel_size, self.vox = oracle, voxel_size, {}

    def insert(self, world, cap):
        keys = self.oracle.voxel_index(self.voxel_size, world)
        for k, p in zip(map(tuple, keys.tolist()), world):
            pts = self.vox.setdefault(k, [])
            if len(pts) < cap:
                pts.append(p)

    def evict(self, position, distance):
        """needsPointRemoval (src/LocalMap.cpp:149-154), evaluated as the device evaluates it."""
        gone = []
        for k in list(self.vox):
            d = [(k[a] + 0.5) * self.voxel_size - position[a] for a in range(3)]
            if np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > distance:
                del self.vox[k]
                gone.append(k)
        return gone

    def erase(self, keys):
        for k in map(tuple, np.asarray(keys).tolist()):
            self.vox.pop(k, None)


def world_of(oracle, points, T):
    return oracle.transform(points, np.tile(np.eye(3).reshape(9), (len(points), 1)), T)[0]


def grouped(keys, points):
    """key -> the exported points of the voxel; asserts that every voxel's points are contiguous."""
    out = {}
    if len(keys) == 0:
        return out
    change = np.any(keys[1:] != keys[:-1], axis=1)
    starts = np.r_[0, np.nonzero(change)[0] + 1]
    ends = np.r_[starts[1:], len(keys)]
    for s, e in zip(starts, ends):
        k = tuple(keys[s].tolist())
        assert k not in out, f"the points of voxel {k} are not contiguous"
        out[k] = points[s:e]
    return out


def assert_matches(ctx, ref):
    keys, pts = ctx.map_points_export()
    got = grouped(keys, pts)
    assert set(got) == set(ref.vox)
    for k, want in ref.vox.items():
        assert np.array_equal(got[k], np.asarray(want)), k
    mk, _, _, counts = ctx.map_export()
    assert len(mk) == len(got)
    for k, c in zip(map(tuple, mk.tolist()), counts.tolist()):
        assert len(got[k]) == c, (k, len(got[k]), c)
    size, capacity = ctx.map_points_size()
    assert size == len(pts) == sum(len(v) for v in ref.vox.values())
    assert capacity >= size
    return capacity


def poses(count, seed, step=0.6):
    from eskf_lio_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for f in range(count):
        xi = [step * f + rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.3), rng.uniform(-0.05, 0.05),
              rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(-0.2, 0.2)]
        out.append(synth.se3_to_SE3(xi))
    return out


def raw_scan(n, seed, extent=12.0):
    from eskf_lio_amd import synth
    return synth.make_lidar_scan(n, seed=seed, extent=extent)


def unit_covs(n):
    return np.tile((0.01 * np.eye(3)).reshape(9), (n, 1))


def run_sort_path(ctx, ref, frames, cap, seed):
    for f, T in enumerate(poses(frames, seed)):
        pts = raw_scan(3_000, seed * 100 + f)
        ctx.map_insert_scan(pts, unit_covs(len(pts)), T, cap)
        ref.insert(world_of(ref.oracle, pts, T), cap)


def run_list_path(ctx, ref, frames, cap, seed, deferred=False):
    for f, T in enumerate(poses(frames, seed)):
        raw = raw_scan(6_000, seed * 100 + f)
        ctx.scan_prepare(raw, None, None, None, PREP_VOXEL, 30)
        prepared, _ = ctx.scan_download()
        if deferred:
            ctx.map_insert_resident_async(T, cap)
        else:
            ctx.map_insert_resident(T, cap)
        ref.insert(world_of(ref.oracle, prepared, T), cap)


def fresh(capi, hint=50_000, device=0):
    ctx = capi.Context(device)
    ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
    ctx.map_reset(VOXEL, hint)
    return ctx


# ---- 1. every path, several caps ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3, 1000])
@pytest.mark.parametrize("path", ["sort", "lists", "deferred"])
def test_points_per_voxel_equal_the_restatement(oracle, path, cap):
    from eskf_lio_amd import capi
    with fresh(capi) as ctx:
        ref = RawMap(oracle, VOXEL)
        if path == "sort":
            run_sort_path(ctx, ref, 4, cap, seed=3)
        else:
            run_list_path(ctx, ref, 4, cap, seed=4, deferred=path == "deferred")
        assert_matches(ctx, ref)
        if cap > 1:   # the rule was exercised: some voxel holds several points, in scan order across frames
            assert max(len(v) for v in ref.vox.values()) > 1


def test_mixed_paths_append_to_the_same_voxels(oracle):
    from eskf_lio_amd import capi
    with fresh(capi) as ctx:
        ref = RawMap(oracle, VOXEL)
        run_list_path(ctx, ref, 2, 5, seed=6)
        run_sort_path(ctx, ref, 2, 5, seed=6)
        run_list_path(ctx, ref, 2, 5, seed=7, deferred=True)
        assert_matches(ctx, ref)


# ---- 2. evict, erase, re-enter ---------------------------------------------------------------------------------------
def test_evicted_and_erased_voxels_lose_their_points_and_start_afresh(oracle):
    from eskf_lio_amd import capi
    with fresh(capi) as ctx:
        ref = RawMap(oracle, VOXEL)
        run_sort_path(ctx, ref, 3, 4, seed=11)
        pos = np.array([1.0, 0.5, 0.0])
        removed = ctx.map_evict(pos, 6.0)
        gone = ref.evict(pos, 6.0)
        assert removed == len(gone) > 0
        keys, _ = ctx.map_points_export()
        assert not set(map(tuple, keys.tolist())) & set(gone)
        assert_matches(ctx, ref)
        # erase a few of the voxels that remain
        victims = np.array(sorted(ref.vox)[:25], dtype=np.int32)
        ctx.map_erase(victims)
        ref.erase(victims)
        assert_matches(ctx, ref)
        # the same scans again: the evicted / erased voxels are re-created from their first points
        run_sort_path(ctx, ref, 3, 4, seed=11)
        assert set(gone) & set(ref.vox) and set(map(tuple, victims.tolist())) & set(ref.vox)
        assert_matches(ctx, ref)
        run_list_path(ctx, ref, 2, 4, seed=12)
        ref.evict(pos, 4.0), ctx.map_evict(pos, 4.0)
        run_list_path(ctx, ref, 2, 4, seed=13, deferred=True)
        assert_matches(ctx, ref)


# ---- 3. growth from nothing ---------------------------------------------------------------------------------------
def test_store_grows_and_survives_rehashes(oracle):
    from eskf_lio_amd import capi
    with fresh(capi, hint=0) as ctx:
        ref = RawMap(oracle, VOXEL)
        slots0 = ctx.map_size()[1]
        cap0 = ctx.map_points_size()[1]
        caps, slot_sizes = [cap0], [slots0]
        for f, T in enumerate(poses(8, seed=21, step=2.0)):
            if f % 2 == 0:
                pts = raw_scan(3_000, 2100 + f)
                ctx.map_insert_scan(pts, unit_covs(len(pts)), T, 6)
                ref.insert(world_of(oracle, pts, T), 6)
            else:
                raw = raw_scan(6_000, 2100 + f)
                ctx.scan_prepare(raw, None, None, None, PREP_VOXEL, 30)
                prepared, _ = ctx.scan_download()
                ctx.map_insert_resident_async(T, 6)
                ref.insert(world_of(oracle, prepared, T), 6)
            if f % 3 == 2:
                pos = T[:3, 3]
                ctx.map_evict(pos, 10.0)
                ref.evict(pos, 10.0)
            caps.append(assert_matches(ctx, ref))
            slot_sizes.append(ctx.map_size()[1])
        assert max(caps) > cap0, caps
        assert max(slot_sizes) > slots0, slot_sizes


# ---- 4. the store off, and what it refuses ----------------------------------------------------------------------------
def test_store_leaves_the_map_bit_equal_and_refuses_what_it_cannot_keep(oracle):
    from eskf_lio_amd import capi
    with fresh(capi) as on, capi.Context(0) as off:
        off.map_reset(VOXEL, 50_000)
        for ctx in (on, off):
            run_sort_path(ctx, RawMap(oracle, VOXEL), 2, 4, seed=31)
            run_list_path(ctx, RawMap(oracle, VOXEL), 2, 4, seed=32)
            run_list_path(ctx, RawMap(oracle, VOXEL), 2, 4, seed=33, deferred=True)
            ctx.map_evict(np.zeros(3), 7.0)
            run_sort_path(ctx, RawMap(oracle, VOXEL), 1, 4, seed=34)
        a, b = on.map_export(), off.map_export()
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert on.map_points_size()[0] == int(a[3].sum())
        # off: NOT_READY
        for call in (off.map_points_size, off.map_points_export):
            with pytest.raises(capi.VgicpError) as e:
                call()
            assert e.value.code == capi.ERR_NOT_READY
        # refusals
        with pytest.raises(capi.VgicpError) as e:
            off.set_option(capi.OPTION_MAP_RAW_POINTS, 1)          # the map holds voxels
        assert e.value.code == capi.ERR_BAD_ARGUMENT
        with pytest.raises(capi.VgicpError) as e:
            on.map_upsert(a[0][:4], a[1][:4], a[2][:4])           # a mirror batch carries no raw points
        assert e.value.code == capi.ERR_BAD_ARGUMENT
        pts = raw_scan(100, 35)
        with pytest.raises(capi.VgicpError) as e:
            on.map_insert_scan(pts, unit_covs(100), np.eye(4), 1 << 32)
        assert e.value.code == capi.ERR_BAD_ARGUMENT
        for x, y in zip(a, on.map_export()):                      # the refusals changed nothing
            assert np.array_equal(x, y)
        # an emptied map takes the option again; a reset map keeps it and starts empty
        off.map_reset(VOXEL, 1_000)
        off.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
        assert off.map_points_size()[0] == 0
        on.map_reset(VOXEL, 1_000)
        assert on.map_points_size()[0] == 0 and on.map_points_export()[0].shape == (0, 3)
        on.set_option(capi.OPTION_MAP_RAW_POINTS, 0)
        on.map_upsert(a[0][:4], a[1][:4], a[2][:4])
        with pytest.raises(capi.VgicpError) as e:
            on.map_points_size()
        assert e.value.code == capi.ERR_NOT_READY


# ---- 5. multi-device context ----------------------------------------------------------------------------------------
def test_multi_device_context_exports_what_one_device_does(oracle):
    from eskf_lio_amd import capi
    with fresh(capi) as one, capi.Context([0, 0]) as two:
        two.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
        two.map_reset(VOXEL, 50_000)
        for ctx in (one, two):
            ref = RawMap(oracle, VOXEL)
            run_sort_path(ctx, ref, 2, 5, seed=41)
            run_list_path(ctx, ref, 2, 5, seed=42)
            run_list_path(ctx, ref, 1, 5, seed=43, deferred=True)
            ctx.map_evict(np.array([2.0, 0.0, 0.0]), 8.0)
            ref.evict(np.array([2.0, 0.0, 0.0]), 8.0)
            assert_matches(ctx, ref)
        k1, p1 = one.map_points_export()
        k2, p2 = two.map_points_export()
        g1, g2 = grouped(k1, p1), grouped(k2, p2)
        assert set(g1) == set(g2)
        for k in g1:
            assert np.array_equal(g1[k], g2[k])
        with pytest.raises(capi.VgicpError) as e:
            two.map_upsert(k1[:2], p1[:2], unit_covs(2))
        assert e.value.code == capi.ERR_BAD_ARGUMENT


# ---- 6. the drop-in classes: save() with the deferred host copy ------------------------------------------------------
def test_drop_in_save_with_deferred_copy_equals_the_host_map(tmp_path):
    """CloudPreprocessor (deferred host copy: the prepared scan never reaches the host) -> ICP -> LocalMap with
    raw_points_on_device, eviction after every insertion: save() writes the very points a host-authoritative LocalMap
    writes when it is fed the same prepared clouds and poses (src/LocalMap.cpp:156-167; PCD lines compared sorted,
    the reference's unordered_map order is not reproduced)."""
    from eskf_lio_amd import host, synth
    frames, cap = 10, 5
    st = synth.make_imu_states(48, seed=61)
    t = synth.make_point_times(8_000, st[1, 0] + 1e-4, st[-3, 0] + 0.4 / 400.0, seed=61, jitter=1e-3)
    ext = synth.se3_to_SE3([0.02, -0.01, 0.03, 0.01, -0.02, 0.005])
    raws = [synth.make_lidar_scan(8_000, seed=610 + f, extent=25.0) for f in range(frames)]
    cfg = dict(translation_sq_threshold=-1.0, cosine_threshold=2.0, remove_distant_points=True,
               distance_threshold=14.0, removing_period=-1.0)
    pre = host.CloudPreprocessor(PREP_VOXEL, ext, "deferred")
    icp = host.ICP(30, 1e-6, 0.9999)
    lmap = host.LocalMap(VOXEL, cap, dict(cfg, device_resident=True, raw_points_on_device=True))
    assert lmap.savesRawPoints()
    pose, trail = np.eye(4), []
    for f, raw in enumerate(raws):
        fr = host.Frame(raw, t, st)
        fr.run(pre, icp, lmap, pose, first_frame=(f == 0))
        got = fr.end()
        pose = got["pose"]
        trail.append(pose)
        if f > 0:
            assert got["used_resident"] and got["host_points"] == raw.shape[0]   # the host cloud was never filled
    assert lmap.savesRawPoints() and lmap.drain() == 0                           # no shadow grid
    lmap.save(str(tmp_path / "dev.pcd"), str(tmp_path / "dev.json"))
    # the same prepared clouds (the preparation is deterministic), the same poses, into a host-authoritative map
    ref = host.LocalMap(VOXEL, cap, dict(cfg, device_resident=False))
    assert ref.savesRawPoints()
    for f, raw in enumerate(raws):
        pts, covs = pre.process(st if f > 0 else np.zeros((0, 8)), raw, t)
        ref.updateLocalMap(pts, covs, trail[f])
    ref.save(str(tmp_path / "ref.pcd"), str(tmp_path / "ref.json"))
    dev = (tmp_path / "dev.pcd").read_text().splitlines()
    want = (tmp_path / "ref.pcd").read_text().splitlines()
    assert dev[:11] == want[:11] and want[9].startswith("POINTS ")              # header: the same number of points
    assert int(want[9].split()[1]) > 1000
    assert sorted(dev[11:]) == sorted(want[11:])


# ---- 7. no new per-frame wait ---------------------------------------------------------------------------------------
def test_resident_chain_keeps_one_sync_per_frame_with_the_store_on(oracle):
    """The steady state of the frame chain: frame k's synchronisation (in align_resident) settles insertion k-1, whose
    totals and log fill travel back with frame k's counter copy.  Nothing else touches the two contexts between their
    frames: the prepared scans for the restatement come from a twin context (same preparation, same bits), which is
    driven outside the counted windows."""
    from eskf_lio_amd import capi, synth
    frames, n, cap = 8, 9_000, 20
    with capi.Context(0) as on, capi.Context(0) as off, capi.Context(0) as twin:
        on.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
        ref = RawMap(oracle, VOXEL)
        for c in (on, off):
            c.map_reset(VOXEL, 400_000)                        # head-room: no rehash and no growth of the store
        results = {}
        for name, c in (("on", on), ("off", off)):
            pose, syncs, out = np.eye(4), [], []
            for f in range(frames):
                raw = synth.make_lidar_scan(n, seed=700 + f, extent=25.0)
                c.frame_stats(reset=True)
                c.scan_prepare_async(raw, None, None, None, PREP_VOXEL, 30)
                if f > 0:
                    guess = pose @ synth.se3_to_SE3([0.01, 0.0, 0.0, 0.0, 0.0, 0.002])
                    pose = c.align_resident(guess, 12, 1e-6, 0.9999).pose
                c.map_insert_resident_async(pose, cap)
                syncs.append(c.frame_stats().host_syncs)
                out.append(pose)
                if name == "on":   # outside the counted window, on another context: `on` keeps its insertion pending
                    twin.scan_prepare(raw, None, None, None, PREP_VOXEL, 30)
                    ref.insert(world_of(oracle, twin.scan_download()[0], pose), cap)
            results[name] = (syncs, out)
        assert results["on"][0] == results["off"][0]
        assert results["on"][0][1:] == [1] * (frames - 1)
        for a, b in zip(results["on"][1], results["off"][1]):
            assert np.array_equal(a, b)
        for x, y in zip(on.map_export(), off.map_export()):
            assert np.array_equal(x, y)
        assert_matches(on, ref)
