"""vgicp_rays_resident (include/vgicp_hip_map_rays.h): the first map voxel on every ray of the resident scan, read-only.

The rule is the header's, restated operation by operation in tests/map_rays_reference.py: every plane and every count is
compared exactly (the rule is written so that the device returns numpy's bits).  tests/test_map_rays_cpu.py checks the
reference on its own, against carving's walk and a brute-force first hit."""
import ctypes as C

import numpy as np
import pytest

import map_rays_reference as mr
from map_rays_reference import MARGIN_BEYOND, ORIGIN, SIZES, STRIDES, VOXEL, Params

pytestmark = pytest.mark.gpu

COUNTER_SCAN_GENERATION = 5
CAP = 20


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def state(ctx, raw=False):
    out = list(ctx.map_export())
    if raw:
        pk, pp = ctx.map_points_export()
        order = np.lexsort(pk.T)
        out += [pk[order], pp[order]]
    return out


def same_state(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def scan_covs(n):
    return np.tile((1e-3 * np.eye(3)).reshape(9), (n, 1))


@pytest.fixture(scope="module")
def scene():
    """The room, the largest scan (every smaller one is its head: a prefix of a scan is a scan) and the pose."""
    return mr.make_scene(max(SIZES))


_references = {}


def reference(keys, pts, T, p: Params, tag="room"):
    """The reference's result, computed once per (map, scan, parameters)."""
    key = (tag, len(keys), len(pts), p.margin, p.beyond, p.max_range, p.stride, p.origin, np.asarray(T).tobytes())
    if key not in _references:
        _references[key] = mr.rays(keys, VOXEL, pts, T, p)
    return _references[key]


def load(ctx, room, hint=None):
    ctx.map_reset(room.voxel_size, len(room.keys) if hint is None else hint)
    ctx.map_upsert(room.keys, room.means, room.covs)


def check(rep, want, what=None):
    """Every plane bit for bit, every count."""
    assert same_bits(rep.status, want.status), what
    assert same_bits(rep.range, want.range), what
    assert same_bits(rep.hit_key, want.hit_key), what
    assert same_bits(rep.steps, want.steps), what
    assert rep.counts == [want.counts()], (what, rep.counts, want.counts())


def poses_around(T, k):
    out = []
    for f in range(k):
        P = np.array(T)
        P[:3, 3] += (0.37 * f, -0.21 * f, 0.05 * f)
        a = 0.03 * f
        P[:3, :3] = P[:3, :3] @ np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        out.append(P)
    return out


# ---- 1: parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_planes_and_counts_are_the_references(gpu_ctx, scene, n):
    room, pts, T = scene[0], scene[1][:n], scene[2]
    load(gpu_ctx, room)
    gpu_ctx.scan_upload(pts, scan_covs(n))
    classes = np.zeros(8, dtype=np.int64)
    for stride in STRIDES:
        for margin, beyond in MARGIN_BEYOND:
            p = Params(margin=margin, beyond=beyond, stride=stride, origin=ORIGIN)
            want = reference(room.keys, pts, T, p)
            rep = gpu_ctx.rays_resident(T, p.as_dict())
            check(rep, want, (n, stride, margin, beyond))
            assert rep.launches == 2 and rep.groups == 1 and rep.device_seconds > 0.0
            classes += want.counts()["by_class"]
    if n >= 63:
        assert np.all(classes[1:7] > 0), classes
    if n == max(SIZES):
        print(f"n {n}: {want.counts()} device {1e6 * rep.device_seconds:.1f} us")


# ---- 2: read-only -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
def test_the_call_changes_nothing(scene, raw):
    from eskf_lio_amd import capi
    room, pts, T = scene[0], scene[1][:1000], scene[2]
    rng = np.random.default_rng(5)
    p = Params(margin=1.0, beyond=20.0, origin=ORIGIN)
    with capi.Context(0) as ctx:
        if raw:
            ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
        ctx.map_reset(VOXEL, len(room.keys))
        p3 = (room.keys + rng.uniform(0.05, 0.95, size=(len(room.keys), 3))) * VOXEL
        ctx.map_insert_scan(p3, room.covs, np.eye(4), CAP)
        ctx.scan_upload(pts, scan_covs(len(pts)))
        guess = np.array(T)
        guess[:3, 3] += (0.05, -0.03, 0.02)
        first = ctx.align_resident(guess, 4, 1e-12, 1.0 - 1e-12, allow_degenerate=True)
        before, generation, size = state(ctx, raw), ctx.counter(COUNTER_SCAN_GENERATION), ctx.map_size()
        rep = ctx.rays_resident(T, p.as_dict())
        many = ctx.rays_resident(poses_around(T, 3), p.as_dict())
        assert rep.counts[0]["rays"] == len(pts) and many.counts[0] == rep.counts[0]
        assert rep.counts == [reference(before[0], pts, T, p, tag="inserted").counts()]
        assert same_state(state(ctx, raw), before) and ctx.map_size() == size
        assert ctx.counter(COUNTER_SCAN_GENERATION) == generation
        second = ctx.align_resident(guess, 4, 1e-12, 1.0 - 1e-12, allow_degenerate=True)
        assert same_bits(first.pose, second.pose) and first.iterations == second.iterations
        assert same_bits(first.normal_eq, second.normal_eq) and same_bits(first.corr_count, second.corr_count)


# ---- 3: several poses -------------------------------------------------------------------------------------------------
def test_five_poses_are_five_single_calls_and_the_reference(gpu_ctx, scene):
    room, pts, T = scene[0], scene[1][:1000], scene[2]
    load(gpu_ctx, room)
    gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
    p = Params(margin=1.0, beyond=20.0, stride=3, origin=ORIGIN)
    poses = poses_around(T, 5)
    rep = gpu_ctx.rays_resident(poses, p.as_dict())
    assert rep.status is None and rep.launches == 2 and rep.groups == 1
    singles = [gpu_ctx.rays_resident(P, p.as_dict(), per_point=False).counts[0] for P in poses]
    want = [mr.rays(room.keys, VOXEL, pts, P, p).counts() for P in poses]
    assert rep.counts == singles == want
    assert len({tuple(c["by_class"]) for c in want}) == 5          # the poses differ


def test_thirty_three_poses_on_a_large_table_go_in_three_groups(gpu_ctx, scene):
    """map_reset(h, 2 000 000): a table of 2^23 slots (1 GiB), a bitmap of 1 MiB per pose, 16 poses per group."""
    room, pts, T = scene[0], scene[1][:65], scene[2]
    load(gpu_ctx, room, 2_000_000)
    assert gpu_ctx.map_size() == (len(room.keys), 1 << 23)
    gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
    p = Params(margin=1.0, beyond=20.0, origin=ORIGIN)
    poses = poses_around(T, 33)
    rep = gpu_ctx.rays_resident(poses, p.as_dict())
    assert rep.groups == 3 and rep.launches == 6
    singles = [gpu_ctx.rays_resident(P, p.as_dict(), per_point=False) for P in poses]
    assert all(s.groups == 1 and s.launches == 2 for s in singles)
    assert rep.counts == [s.counts[0] for s in singles]
    assert rep.counts[::8] == [mr.rays(room.keys, VOXEL, pts, P, p).counts() for P in poses[::8]]
    check(gpu_ctx.rays_resident(T, p.as_dict()), reference(room.keys, pts, T, p))


# ---- 4: tables that have lived ----------------------------------------------------------------------------------------
def test_tombstones_on_the_walked_paths_and_a_rehash(gpu_ctx, scene):
    from eskf_lio_amd import synth
    room, pts, T = scene[0], scene[1][:1000], scene[2]
    load(gpu_ctx, room)
    slots = gpu_ctx.map_size()[1]
    gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
    p = Params(margin=1.0, beyond=20.0, origin=ORIGIN)
    check(gpu_ctx.rays_resident(T, p.as_dict()), reference(room.keys, pts, T, p))
    # half of the room evicted: tombstones where the walks probe
    removed = gpu_ctx.map_evict((-12.0, 0.0, 0.0), 17.0)
    left = gpu_ctx.map_export()[0]
    assert 0.3 * len(room.keys) < removed < 0.7 * len(room.keys) and gpu_ctx.map_size() == (len(left), slots)
    want = mr.rays(left, VOXEL, pts, T, p)
    check(gpu_ctx.rays_resident(T, p.as_dict()), want, "evicted")
    assert want.counts()["by_class"][mr.OPEN] > reference(room.keys, pts, T, p).counts()["by_class"][mr.OPEN]
    # an insertion that forces a rehash: another table, another bitmap
    more = synth.make_map(30_000, voxel_size=VOXEL)
    gpu_ctx.map_upsert(more.keys + np.array([500, 0, 0], dtype=np.int32), more.means, more.covs)
    assert gpu_ctx.map_size()[1] > slots
    grown = gpu_ctx.map_export()[0]
    assert len(grown) == len(left) + 30_000
    check(gpu_ctx.rays_resident(T, p.as_dict()), mr.rays(grown, VOXEL, pts, T, p), "rehashed")


# ---- 5: corners of the rule -------------------------------------------------------------------------------------------
def corner_map(keys):
    keys = np.asarray(keys, dtype=np.int32).reshape(-1, 3)
    return mr.Room(VOXEL, keys, (keys.astype(np.float64) + 0.5) * VOXEL, np.tile((1e-3 * np.eye(3)).reshape(9), (len(keys), 1)), keys[:0])


def test_corners_of_the_rule(gpu_ctx):
    nan, inf = float("nan"), float("inf")
    room = corner_map([[4, 0, 0], [0, 6, 0], [2, 2, 2], [0, 0, -5], [-3, 0, 0]])
    pts = np.array([[2.75, 0.25, 0.25],      # along +x (d_y = d_z = 0): through voxel 4
                    [0.25, 3.75, 0.25],      # along +y
                    [0.25, 0.25, -3.0],      # along -z: behind voxel -5
                    [1.25, 1.25, 1.25],      # the diagonal into its own voxel (2, 2, 2)
                    [0.25, 0.25, 0.25],      # a point at the origin: len = 0
                    [nan, 0.25, 0.25], [0.25, inf, 0.25], [0.25, 0.25, -inf],
                    [2.25, 0.25, 0.25],      # in voxel 4
                    [-1.75, 0.3, 0.3]])      # behind voxel -3
    load(gpu_ctx, room)
    gpu_ctx.scan_upload(pts, scan_covs(len(pts)))
    eye = np.eye(4)
    p = Params(margin=0.3, beyond=1.0, origin=(0.25, 0.25, 0.25))
    want = mr.rays(room.keys, VOXEL, pts, eye, p)
    assert want.status.tolist() == [mr.CONFIRMED, mr.BLOCKED, mr.BLOCKED, mr.OWN, mr.NO_RAY, mr.NO_RAY, mr.NO_RAY, mr.NO_RAY,
                                    mr.OWN, mr.BLOCKED]
    assert want.steps.tolist() == [5, 7, 6, 7, 0, 0, 0, 0, 5, 4] and want.range[:3].tolist() == [1.75, 2.75, 2.25]
    check(gpu_ctx.rays_resident(eye, p.as_dict()), want, "axes")
    # the diagonal from a voxel's corner: every step a three-way tie, x before y before z; the return at (0.25, 0.25, 0.25)
    # lies on it, in front of the voxel
    corner = Params(beyond=2.0, origin=(0.0, 0.0, 0.0))
    want = mr.rays(room.keys, VOXEL, pts, eye, corner)
    assert want.status[3] == mr.OWN and want.status[4] == mr.BEHIND and want.steps[3] == want.steps[4] == 7
    assert want.hit_key[3].tolist() == want.hit_key[4].tolist() == [2, 2, 2]
    check(gpu_ctx.rays_resident(eye, corner.as_dict()), want, "corner")
    # a FULL voxel at key(o): t_in = 0, range 0, not OWN (but OWN for the return inside it)
    inside = Params(beyond=1.0, origin=(2.3, 0.2, 0.1))
    want = mr.rays(room.keys, VOXEL, pts, eye, inside)
    assert want.status[0] == mr.CONFIRMED and want.status[8] == mr.OWN and want.range[0] == 0.0 and want.steps[0] == 1
    check(gpu_ctx.rays_resident(eye, inside.as_dict()), want, "key(o) is FULL")
    # max_range shorter than the return
    short = Params(beyond=1.0, max_range=1.0, origin=(0.25, 0.25, 0.25))
    want = mr.rays(room.keys, VOXEL, pts, eye, short)
    assert want.status[0] == mr.OPEN and want.steps[0] == 3
    check(gpu_ctx.rays_resident(eye, short.as_dict()), want, "max_range")
    # a pose that puts key(o) out of range: every point NO_RAY, not refused
    far = np.eye(4)
    far[0, 3] = 2.0 ** 30
    rep = gpu_ctx.rays_resident(far, p.as_dict())
    check(rep, mr.rays(room.keys, VOXEL, pts, far, p), "key(o) undefined")
    assert rep.counts[0]["by_class"] == [len(pts), 0, 0, 0, 0, 0, 0, 0] and rep.counts[0]["rays"] == 0 and not rep.steps.any()
    # an empty map: every ray OPEN
    gpu_ctx.map_reset(VOXEL, 0)
    rep = gpu_ctx.rays_resident(eye, p.as_dict())
    check(rep, mr.rays(np.zeros((0, 3), dtype=np.int64), VOXEL, pts, eye, p), "empty map")
    assert rep.counts[0]["by_class"] == [4, 6, 0, 0, 0, 0, 0, 0]
    # an empty scan: OK, zero counts, no launch
    gpu_ctx.scan_upload(np.zeros((0, 3)), np.zeros((0, 9)))
    rep = gpu_ctx.rays_resident([eye, eye], p.as_dict())
    assert rep.counts == [dict(rays=0, visits=0, by_class=[0] * 8)] * 2 and rep.launches == 0 and rep.groups == 0


# ---- 6: refusals and optional planes ----------------------------------------------------------------------------------
def test_refusals_in_their_order_leave_the_outputs_alone(scene):
    from eskf_lio_amd import capi
    room, pts, T = scene[0], scene[1][:300], scene[2]
    lib = capi.load_library()
    n = len(pts)
    good = np.stack([capi.pose_to_abi(P) for P in poses_around(T, 2)])
    bad = good.copy()
    bad[1, 13] = np.inf
    status, rng = np.zeros(n, dtype=np.uint8), np.zeros(n)
    keys, steps = np.zeros((n, 3), dtype=np.int32), np.zeros(n, dtype=np.uint32)
    counts, stats = (capi.RayCounts * 64)(), capi.RayStats()
    nan, inf = float("nan"), float("inf")
    dp = C.POINTER(C.c_double)

    def fill():
        status[:] = 0x5A
        rng[:] = -7.0
        keys[:] = 0x5A5A5A5A
        steps[:] = 0x5A5A5A5A
        C.memset(counts, 0xA5, C.sizeof(counts))
        C.memset(C.byref(stats), 0xA5, C.sizeof(stats))

    def untouched():
        return (np.all(status == 0x5A) and np.all(rng == -7.0) and np.all(keys == 0x5A5A5A5A) and np.all(steps == 0x5A5A5A5A) and
                bytes(counts) == b"\xa5" * C.sizeof(counts) and bytes(stats) == b"\xa5" * C.sizeof(stats))

    def call(ctx, poses=good, k=1, with_params=True, planes=True, reserved=0, **kw):
        fill()
        rp = capi.ray_params(**dict(Params(origin=ORIGIN).as_dict(), **kw))
        rp.reserved = reserved
        out = capi.RayOutputs(status.ctypes.data_as(C.POINTER(C.c_uint8)), rng.ctypes.data_as(dp),
                              keys.ctypes.data_as(C.POINTER(C.c_int32)), steps.ctypes.data_as(C.POINTER(C.c_uint32)))
        return lib.vgicp_rays_resident(ctx._h if ctx is not None else None, poses.ctypes.data_as(dp) if poses is not None else None, k,
                                       C.byref(rp) if with_params else None, C.byref(out) if planes else None, counts, C.byref(stats))

    assert call(None) == capi.ERR_BAD_ARGUMENT and untouched()                                              # 1
    with capi.Context(0) as ctx:
        # 3 in front of everything behind it
        assert call(ctx, poses=None, with_params=False) == capi.ERR_NOT_READY and "map" in ctx.last_error() and untouched()
        load(ctx, room)
        assert call(ctx, poses=None, margin=nan) == capi.ERR_NOT_READY and "scan" in ctx.last_error() and untouched()
        ctx.scan_upload(pts, scan_covs(n))
        before, generation = state(ctx), ctx.counter(COUNTER_SCAN_GENERATION)

        def refused(text, **kwargs):
            assert call(ctx, **kwargs) == capi.ERR_BAD_ARGUMENT and text in ctx.last_error(), (kwargs, ctx.last_error())
            assert untouched()

        refused("n_poses", poses=None, margin=nan)                                                           # 4
        refused("n_poses", with_params=False, poses=bad, k=2)
        refused("n_poses", k=0, poses=bad)
        refused("n_poses", k=65, margin=nan)
        refused("not finite", poses=bad, k=2, planes=False, margin=nan)                                      # 5 before 6
        refused("not finite", origin=(0.0, nan, 0.0), margin=-1.0)
        assert call(ctx, poses=bad, k=1) == capi.OK                                                          # (only the first pose is read)
        for margin in (nan, -1.0, -1e-300, inf, -inf):                                                       # 6 before 7
            refused("margin must be", margin=margin, beyond=nan)
        for beyond in (nan, -1.0, -1e-300, inf, -inf):                                                       # 7 before 8
            refused("beyond must be", beyond=beyond, max_range=nan)
        for max_range in (nan, 0.0, -1.0, inf, 4096.5 * VOXEL):                                              # 8 before 9
            refused("max_range must be", max_range=max_range, stride=0)
        refused("stride must be", stride=0, k=2)                                                             # 9 before 10
        refused("stride must be", reserved=1, k=2)
        refused("single pose", k=2)                                                                          # 10
        # 11: a communicator (one rank is enough) behind 10
        ctx.comm_init(1, 0, ctx.comm_unique_id())
        refused("single pose", k=2)
        refused("single-device")
        refused("single-device", k=2, planes=False)
        ctx.comm_destroy()
        assert same_state(state(ctx), before) and ctx.counter(COUNTER_SCAN_GENERATION) == generation
        assert call(ctx, max_range=4096.0 * VOXEL) == capi.OK and not untouched()
        assert call(ctx, k=2, planes=False) == capi.OK and np.all(status == 0x5A) and counts[1].rays == n
    with capi.Context([0, 0]) as multi:                                                                      # 11
        assert call(multi) == capi.ERR_NOT_READY                       # 3 before 11: no map
        load(multi, room)
        multi.scan_upload(pts, scan_covs(n))
        assert call(multi) == capi.ERR_BAD_ARGUMENT and "single-device" in multi.last_error() and untouched()


def test_planes_left_out_one_at_a_time_leave_the_others_equal(gpu_ctx, scene):
    from eskf_lio_amd import capi
    room, pts, T = scene[0], scene[1][:1000], scene[2]
    lib = capi.load_library()
    n = len(pts)
    load(gpu_ctx, room)
    gpu_ctx.scan_upload(pts, scan_covs(n))
    p = Params(margin=1.0, beyond=20.0, stride=3, origin=ORIGIN)
    want = reference(room.keys, pts, T, p)
    whole = dict(status=want.status, range=want.range, hit_key=want.hit_key, steps=want.steps)
    pose, rp = capi.pose_to_abi(T), capi.ray_params(**p.as_dict())
    types = dict(status=C.c_uint8, range=C.c_double, hit_key=C.c_int32, steps=C.c_uint32)
    for without in (None, "status", "range", "hit_key", "steps"):
        got = {name: np.zeros_like(a) for name, a in whole.items()}
        out = capi.RayOutputs(*[None if name == without else got[name].ctypes.data_as(C.POINTER(types[name]))
                                for name in ("status", "range", "hit_key", "steps")])
        counts = capi.RayCounts()
        assert lib.vgicp_rays_resident(gpu_ctx._h, pose.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(rp), C.byref(out),
                                       C.byref(counts), None) == capi.OK
        for name, a in whole.items():
            assert same_bits(got[name], np.zeros_like(a) if name == without else a), (without, name)
        assert counts.rays == want.counts()["rays"] and list(counts.by_class) == want.counts()["by_class"]
    # no counts, no stats, no planes: still fine
    assert lib.vgicp_rays_resident(gpu_ctx._h, pose.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(rp), None, None, None) == capi.OK


# ---- 7: the layers above ----------------------------------------------------------------------------------------------
def test_drop_in_report_is_the_abi_chains():
    """CloudPreprocessor::process -> ICP::align -> LocalMap::updateLocalMap through the C++ classes, then
    LocalMap::rayReport / rayCounts at the frame's pose: the planes and counts of vgicp_rays_resident behind the same chain
    on the bare C ABI.  A host-authoritative map has no report: not available, nothing raised."""
    from eskf_lio_amd import capi, host
    from test_multi_device import _NO_GATE, _frame_inputs
    st, t, ext, raws = _frame_inputs(frames=2, n=20_000)
    rays = dict(margin=0.3, beyond=5.0, max_range=30.0, stride=2, origin=tuple(ext[:3, 3]))
    with capi.Context(0) as c:
        c.map_reset(0.3, 0)
        pose = np.eye(4)
        for f, raw in enumerate(raws):
            c.scan_prepare_async(raw, t if f else None, st if f else None, ext, 0.3, 30)
            if f > 0:
                pose = c.align_resident(pose, 30, 1e-6, 0.9999).pose
            c.map_insert_resident_async(pose, CAP)
        want = c.rays_resident(pose, rays)
        others = poses_around(pose, 3)
        want_counts = c.rays_resident(others, rays).counts
    assert want.counts[0]["rays"] > 1000 and sum(want.counts[0]["by_class"][1:]) == want.counts[0]["rays"]
    assert want_counts[0] == want.counts[0] and len(want_counts) == 3

    pre = host.CloudPreprocessor(0.3, ext, "deferred")
    icp = host.ICP(30, 1e-6, 0.9999)
    lmap = host.LocalMap(0.3, CAP, dict(_NO_GATE, device_resident=True))
    got_pose = np.eye(4)
    for f, raw in enumerate(raws):
        fr = host.Frame(raw, t, st)
        fr.run(pre, icp, lmap, got_pose, first_frame=(f == 0))
        got = fr.end()
        if f > 0:
            got_pose = got["pose"]
    assert np.array_equal(got_pose, pose)
    rep = lmap.rayReport(got_pose, **rays)
    assert rep is not None and rep["counts"] == want.counts[0]
    for name in ("status", "range", "hit_key", "steps"):
        assert same_bits(rep[name], getattr(want, name)), name
    assert lmap.rayCounts(others, **rays) == want_counts
    assert host.LocalMap(0.3, CAP).rayReport(got_pose, **rays) is None
    assert host.LocalMap(0.3, CAP).rayCounts(others, **rays) is None


def test_replay_reports_at_every_aligned_pose():
    """tools/replay.py --resident --ray-report: the class totals of the run are in the summary it returns, one report per
    aligned frame, and the trajectory is the one without the flag (the report is read-only)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(root, "tools", "replay.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        base = ["--synthetic", "4", "--points", "6000", "--resident"]
        plain = tool.main(base + ["--out", os.path.join(tmp, "plain.tum")])
        summary = tool.main(base + ["--out", os.path.join(tmp, "rays.tum"), "--ray-report", "30", "--ray-margin", "0.3",
                                    "--ray-beyond", "5", "--ray-stride", "2"])
        assert open(os.path.join(tmp, "plain.tum")).read() == open(os.path.join(tmp, "rays.tum")).read()
    assert plain["ray_report"] is None and summary["poses"] == plain["poses"] == 4
    rep = summary["ray_report"]
    assert rep["frames"] == 3 and rep["rays"] > 1000 and sum(rep["by_class"][1:]) == rep["rays"]
    assert rep["classes"]["no_ray"] == rep["by_class"][0] > 0 and rep["visits"] >= rep["rays"]          # (stride 2)
