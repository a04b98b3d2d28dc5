"""-m gpu: the entry points that insert a scan into the voxel map — vgicp_map_insert_scan, vgicp_map_insert_resident,
vgicp_map_insert_resident_async and the two forms a multi-device context inserts its resident scan by — held against
each other: the same scan at the same pose gives the same map byte for byte whichever way it came, and each entry
refuses what it refuses with its own status and text, in its own order of checks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PREP_VOXEL = 0.3
POSE_XI = [0.4, -0.3, 0.2, 0.03, -0.02, 0.05]   # not the identity: the points change voxels on their way into the map
NO_MAP = "no voxel map: call vgicp_map_reset first"
NO_SCAN = "no scan resident: call vgicp_scan_upload first"
NULL_POINTER = "NULL pointer"
CAP_ZERO = "max_points_per_voxel must be >= 1"
CAP_RAW = "max_points_per_voxel must be < 2^32 while the map keeps raw points"


@pytest.fixture(scope="module")
def rig():
    """One single-device context and one group of two sub-contexts on the one device, the same sweep prepared at 0.3 m and
    resident in both; the prepared scan fetched ONCE.  A map_reset leaves the resident scan alone."""
    from eskf_lio_amd import capi, synth
    raw = synth.make_lidar_scan(3000, seed=41, extent=30.0)
    one, group = capi.Context(0), capi.Context([0, 0])
    try:
        one.scan_prepare_async(raw, None, None, None, PREP_VOXEL, 30)
        pts, covs = one.scan_fetch()
        assert 512 < len(pts) <= 3000
        assert group.scan_prepare(raw, None, None, None, PREP_VOXEL, 30)[0] == len(pts)
        pts.setflags(write=False)
        covs.setflags(write=False)
        yield one, group, pts, covs
    finally:
        group.close()
        one.close()


def _record(ctx, new, raw_on):
    """what an insertion into a fresh map left: the counts, the voxels sorted by key, the raw points sorted"""
    voxels, slots = ctx.map_size()
    assert new is None or new == voxels            # the map was empty: every voxel is a new one
    out = [voxels, slots, *ctx.map_export()]
    if raw_on:
        keys, points = ctx.map_points_export()
        order = np.lexsort((points[:, 2], points[:, 1], points[:, 0], keys[:, 2], keys[:, 1], keys[:, 0]))
        out += [keys[order], points[order]]
    return out


def _same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


@pytest.mark.parametrize("map_voxel", [0.3, 1.5])   # (ceil(map / scan voxel) + 1)^3 = 8: short lists; 216 > 64: the sort
@pytest.mark.parametrize("raw_on", [False, True])
@pytest.mark.parametrize("cap", [1, 20])
def test_every_route_builds_the_same_map(rig, cap, raw_on, map_voxel):
    """The prepared scan of a 3 000-point sweep goes, at one pose, into a fresh 1024-slot map (more than 512 points: the
    table grows inside the insertion) through vgicp_map_insert_scan, vgicp_map_insert_resident,
    vgicp_map_insert_resident_async + vgicp_map_size, and the synchronous and the deferred resident insertion of a group of
    two sub-contexts (raw points off only: a group keeps them on its first device).  new_voxels, vgicp_map_size, the
    exported voxels sorted by key and (raw points on) the exported points sorted are identical, arrays byte for byte."""
    from eskf_lio_amd import capi, synth
    one, group, pts, covs = rig
    T = synth.se3_to_SE3(POSE_XI)
    routes = [("insert_scan", one, lambda: one.map_insert_scan(pts, covs, T, cap)),
              ("insert_resident", one, lambda: one.map_insert_resident(T, cap)),
              ("insert_resident_async", one, lambda: one.map_insert_resident_async(T, cap))]
    if not raw_on:
        routes += [("group insert_resident", group, lambda: group.map_insert_resident(T, cap)),
                   ("group insert_resident_async", group, lambda: group.map_insert_resident_async(T, cap))]
    one.map_reset(map_voxel, 0)                    # the option is switched on an empty map only
    one.set_option(capi.OPTION_MAP_RAW_POINTS, int(raw_on))
    records = {}
    for name, ctx, insert in routes:
        ctx.map_reset(map_voxel, 0)
        assert ctx.map_size() == (0, 1024)
        records[name] = _record(ctx, insert(), raw_on)
    first = records["insert_scan"]
    assert 0 < first[0] <= len(pts) and first[1] > 1024 and int(first[5].sum()) <= cap * first[0]
    if raw_on:
        assert len(first[7]) == int(first[5].sum())
    for name, rec in records.items():
        differ = [i for i, (x, y) in enumerate(zip(first, rec)) if not _same(x, y)]
        assert len(rec) == len(first) and not differ, (name, differ)


def test_each_entry_refuses_in_its_own_order(rig):
    """Status and text of every entry for: no map; no resident scan; a NULL transform; a cap of 0; a cap of 2^32 with raw
    points on; an empty scan with a NULL transform (the upload entry looks at n first and accepts, the others refuse);
    and a deferred insertion followed at once by a synchronous one, which settles the first inside the second."""
    from eskf_lio_amd import capi, synth
    lib = capi.load_library()
    _, _, pts, covs = rig
    n = len(pts)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    T_abi = capi.pose_to_abi(synth.se3_to_SE3(POSE_XI))
    new = C.c_size_t(77)

    def scan(c, T, cap, count=n):
        return lib.vgicp_map_insert_scan(c._h, count, dp(pts) if count else None, dp(covs) if count else None, T, cap, C.byref(new))

    def resident(c, T, cap):
        return lib.vgicp_map_insert_resident(c._h, T, cap, C.byref(new))

    def deferred(c, T, cap):
        return lib.vgicp_map_insert_resident_async(c._h, T, cap)

    def refused(call, c, T, cap, code, text):
        new.value = 77
        assert call(c, T, cap) == code, (call.__name__, c.last_error())
        assert c.last_error().endswith(text), (call.__name__, c.last_error())   # a group puts the device in front
        assert call is deferred or new.value == 0

    with capi.Context(0) as one, capi.Context([0, 0]) as group:
        T = dp(T_abi)
        # no map; on one device that is looked at first: before the scan, the transform and the cap
        for call in (scan, resident, deferred):
            refused(call, one, None, 0, capi.ERR_NOT_READY, NO_MAP)
        refused(scan, group, T, 20, capi.ERR_NOT_READY, NO_MAP)
        assert scan(one, None, 0, 0) == capi.ERR_NOT_READY and one.last_error() == NO_MAP   # an empty scan needs a map too
        group.scan_upload(pts, covs)
        for call in (resident, deferred):
            refused(call, group, T, 20, capi.ERR_NOT_READY, NO_MAP)
        # no resident scan: before the transform and the cap
        one.map_reset(1.5, 0)
        for call in (resident, deferred):
            refused(call, one, None, 0, capi.ERR_NOT_READY, NO_SCAN)
        one.scan_upload(pts, covs)
        group.map_reset(1.5, 0)
        for c in (one, group):
            for call in (scan, resident, deferred):
                refused(call, c, None, 0, capi.ERR_BAD_ARGUMENT, NULL_POINTER)   # the transform before the cap
                refused(call, c, T, 0, capi.ERR_BAD_ARGUMENT, CAP_ZERO)
            assert c.map_size() == (0, 1024)                                        # the refusals changed nothing
        # 2^32 points per voxel: accepted, unless the map keeps raw points (their ordinals are 32-bit)
        for c in (one, group):
            c.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
            for call in (scan, resident, deferred):
                refused(call, c, T, 1 << 32, capi.ERR_BAD_ARGUMENT, CAP_RAW)
        assert one.map_size() == (0, 1024)
        group.map_reset(1.5, 0)                    # (its second replica keeps no raw points and took the scans)
        for c in (one, group):
            c.set_option(capi.OPTION_MAP_RAW_POINTS, 0)
        assert resident(one, T, 1 << 32) == capi.OK and new.value == one.map_size()[0] > 0
        # an empty scan: the upload entry returns before it looks at the transform or the cap, the others do not
        empty = np.zeros((0, 3)), np.zeros((0, 9))
        for c in (one, group):
            c.map_reset(1.5, 0)
            c.scan_upload(*empty)
            new.value = 77
            assert scan(c, None, 0, 0) == capi.OK and new.value == 0
            for call in (resident, deferred):
                refused(call, c, None, 20, capi.ERR_BAD_ARGUMENT, NULL_POINTER)
            for call in (resident, deferred):
                new.value = 77
                assert call(c, T, 20) == capi.OK and (call is deferred or new.value == 0)
        for call in (resident, deferred):
            refused(call, one, T, 0, capi.ERR_BAD_ARGUMENT, CAP_ZERO)
        assert one.map_size() == (0, 1024) and group.map_size() == (0, 1024)
        # deferred, then synchronous at once: the second call settles the first.  Against two synchronous insertions.
        T2_abi = capi.pose_to_abi(synth.se3_to_SE3([-0.2, 0.5, 0.1, -0.01, 0.02, 0.3]))
        T2 = dp(T2_abi)
        maps = []
        for c in (one, group):
            c.scan_upload(pts, covs)
            for first, second in ((resident, resident), (deferred, resident), (deferred, scan), (deferred, deferred)):
                c.map_reset(1.5, 0)
                assert first(c, T, 2) == capi.OK and second(c, T2, 2) == capi.OK
                maps.append([*c.map_size(), *c.map_export()])
        assert maps[0][0] > 0
        for m in maps[1:]:
            assert all(_same(x, y) for x, y in zip(maps[0], m))
