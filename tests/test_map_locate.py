"""vgicp_locate_resident (include/vgicp_hip_map_locate.h) on the device: up to 64 poses of the resident scan scored over a
window of whole-voxel shifts on a level of the map, read-only.

Every comparison is `==` against the numpy restatement of the rule (tests/map_locate_reference.py, checked on its own by
tests/test_map_locate_cpu.py) applied to what the device itself exports: the level's keys (map_level_export) and the
downloaded scan.  Every count is an integer, so nothing here has a tolerance but the pipeline's distance to P*, whose
limits are the levels test's."""
import ctypes as C

import numpy as np
import pytest

import map_levels_reference as ml
import map_locate_reference as lo
from conftest import pose_error
from test_map_levels import crafted_keys, fill, random_keys

pytestmark = pytest.mark.gpu

VOXEL = ml.VOXEL
COUNTER_SCAN_GENERATION = 5
SIZES = (1, 63, 64, 65, 449, 1500)


def scan_covs(n):
    return np.tile((1e-3 * np.eye(3)).reshape(9), (n, 1))


def tilted():
    """A full SE(3) pose: a rotation about a skew axis and a translation off every voxel face."""
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    a = 0.4
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)
    T[:3, 3] = (0.731, -1.377, 0.213)
    return T


def yaw(deg, t=(0.0, 0.0, 0.0)):
    return lo.wrong_guess(t, deg)


POSES = (np.eye(4), yaw(30.0), tilted())


@pytest.fixture(scope="module")
def lidar():
    """A 6 000-point map and the largest scan (every smaller one is its head)."""
    from eskf_lio_amd import synth
    return synth.make_lidar_scan(6000, seed=1), synth.make_lidar_scan(6000, seed=2)[:max(SIZES)]


def load_lidar(ctx, lidar, n, levels=3):
    ctx.map_reset(VOXEL, 6000)
    ctx.map_insert_scan(lidar[0], scan_covs(len(lidar[0])), np.eye(4), 20)
    ctx.scan_upload(lidar[1][:n], scan_covs(n))
    if levels:
        ctx.map_levels_build(levels)


_keysets = {}


def check(ctx, poses, level, window, stride=1, what=None, tag=None):
    """The call against the restatement over what the device exports; -> (LocateResult, [Best]).  tag: a name under which
    the level's key set may be kept between calls (the map must not change under one tag)."""
    keys = None
    if tag is None or (tag, level) not in _keysets:
        keys = lo.KeySet(ctx.map_level_export(level)[0])
        if tag is not None:
            _keysets[(tag, level)] = keys
    keys = keys if keys is not None else _keysets[(tag, level)]
    pts = ctx.scan_download()[0]
    h = VOXEL * 2 ** level
    assert ctx.map_level_size(level)[2] == h
    want, plane = lo.locate(keys, h, pts, poses, window, stride)
    got = ctx.locate_resident(poses, level, window, stride)
    assert got.hits.dtype == np.uint32 and got.hits.shape == plane.shape and got.cells == plane.shape[1], what
    assert np.array_equal(got.hits, plane), (what, int((got.hits != plane).sum()))
    for b, w in zip(got.best, want):
        assert {k: v for k, v in b.items() if k != "pose"} == w.as_dict(), (what, b, w)
        assert b["pose"].tobytes() == w.pose.tobytes(), what
        assert b["points"] + b["skipped"] == -(-len(pts) // stride)
    return got, want


# ---- shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_hits_and_bests_are_the_rules_at_every_size_stride_and_level(gpu_ctx, lidar, n):
    load_lidar(gpu_ctx, lidar, n)
    total = 0
    for level in range(4):
        for stride in (1, 3, max(n, 7)):          # the last leaves point 0 alone
            for window in ((0, 0, 0), (2, 1, 0)):
                got, _ = check(gpu_ctx, POSES, level, window, stride, (n, level, stride, window), tag="lidar")
                assert got.launches == 2 and got.device_seconds > 0.0
                total += int(got.hits.sum())
    assert total > 0


@pytest.mark.parametrize("window", ((5, 0, 0), (0, 5, 0), (0, 0, 5), (31, 0, 0), (32, 0, 0), (10, 10, 4)))
def test_windows_one_axis_at_a_time_either_side_of_a_wave_and_the_largest(gpu_ctx, lidar, window):
    load_lidar(gpu_ctx, lidar, 449)
    for level, k in ((0, 1), (1, 2), (3, 2)):
        got, want = check(gpu_ctx, POSES[:k], level, window, 1, (window, level), tag="lidar")
        assert got.cells == (2 * window[0] + 1) * (2 * window[1] + 1) * (2 * window[2] + 1)
    assert max(w.hits for w in want) > 0


def test_a_fan_of_64_yaws(gpu_ctx, lidar):
    load_lidar(gpu_ctx, lidar, 1500)
    fan = lo.yaw_fan(yaw(11.0, (1.3, -0.7, 0.1)), 64)
    got, want = check(gpu_ctx, fan, 3, (4, 4, 1), 1, "fan", tag="lidar")
    assert lo.ranking(got.best) == lo.ranking(want) and len({b["hits"] for b in got.best}) > 8
    print(f"64 poses x 81 cells x 1500 points at level 3: device {1e6 * got.device_seconds:.1f} us")
    again = gpu_ctx.locate_resident(fan, 3, (4, 4, 1))
    assert np.array_equal(again.hits, got.hits) and again.launches == 2          # two calls: equal planes


def test_points_carried_beyond_2_to_the_30_voxels_are_skipped_and_counted(gpu_ctx, lidar):
    load_lidar(gpu_ctx, lidar, 449)
    edge = float(2 ** 30) * VOXEL
    some = np.eye(4)
    some[0, 3] = edge - 2.0          # the points with x above some 2.3 m leave the keys' range at level 0
    every = np.eye(4)
    every[1, 3] = -8.0 * edge
    got, want = check(gpu_ctx, [np.eye(4), some, every], 0, (1, 1, 0), 1, "beyond", tag="lidar")
    assert [b["skipped"] for b in got.best][0] == 0 and 0 < got.best[1]["skipped"] < 449 and got.best[2]["skipped"] == 449
    assert got.best[2]["hits"] == 0 and got.best[2]["cell"] == 0 and got.best[2]["points"] == 0
    got, _ = check(gpu_ctx, [some], 3, (1, 1, 0), 1, "beyond, level 3", tag="lidar")          # 8 times the room at level 3
    assert got.best[0]["skipped"] == 0


# ---- maps --------------------------------------------------------------------------------------------------------------
def test_an_empty_map_and_a_map_of_one_voxel(gpu_ctx, lidar):
    gpu_ctx.map_reset(VOXEL, 100)
    gpu_ctx.scan_upload(lidar[1][:449], scan_covs(449))
    gpu_ctx.map_levels_build(2)
    for level in (0, 2):
        got, _ = check(gpu_ctx, POSES, level, (2, 2, 1), 1, ("empty", level))
        assert not got.hits.any() and all(b["hits"] == 0 and b["cell"] == 0 and b["offset"] == (-2, -2, -1) for b in got.best)
    p = lidar[1][5]
    key = np.floor(p / VOXEL).astype(np.int32).reshape(1, 3)
    gpu_ctx.map_upsert(key, (key + 0.5) * VOXEL, (1e-3 * np.eye(3)).reshape(1, 9))
    for level in (0, 1, 2):
        got, _ = check(gpu_ctx, [np.eye(4)], level, (2, 2, 1), 1, ("one voxel", level))
        assert got.hits[0, got.cells // 2] >= 1          # the centre cell is the shift 0


def test_keys_on_both_sides_of_zero_and_keys_that_collide_in_both_tables(gpu_ctx):
    keys = random_keys(2400, 9, seed=21)
    pts, covs = fill(gpu_ctx, keys, np.ones(len(keys), dtype=np.int64), 1000)
    gpu_ctx.scan_upload(pts[:1500], covs[:1500])
    gpu_ctx.map_levels_build(3)
    for level in range(4):
        got, _ = check(gpu_ctx, POSES, level, (3, 2, 1), 1, ("straddling", level))
    keys, fam_fine, fam_parents, fine_slots, level_slots = crafted_keys()
    pts, covs = fill(gpu_ctx, keys, np.ones(len(keys), dtype=np.int64), 1000, hint=1000)
    gpu_ctx.scan_upload(pts, covs)
    st = gpu_ctx.map_levels_build(3)
    assert st.slots[0] == fine_slots and st.slots[1] == level_slots          # the masks the families were crafted for
    for level in (0, 1):
        got, _ = check(gpu_ctx, [np.eye(4), yaw(3.0)], level, (2, 2, 2), 1, ("crafted", level))
        assert got.best[0]["hits"] == len(pts) and got.best[0]["offset"] == (0, 0, 0)          # every point is in its voxel


def test_a_tombstone_is_never_hit(gpu_ctx):
    keys = random_keys(2400, 9, seed=21)
    pts, covs = fill(gpu_ctx, keys, np.random.default_rng(22).integers(1, 5, size=len(keys)), 1000)
    gpu_ctx.scan_upload(pts[:1500], covs[:1500])
    gpu_ctx.map_levels_build(3)
    before = gpu_ctx.locate_resident(POSES, 0, (2, 2, 1)).hits
    assert 100 < gpu_ctx.map_evict(np.array([1.5, 0.0, 0.0]), 1.6) < len(keys) - 100
    for level in (0, 2):
        got, _ = check(gpu_ctx, POSES, level, (2, 2, 1), 1, ("evicted", level))
    assert int(gpu_ctx.locate_resident(POSES, 0, (2, 2, 1)).hits.sum()) < int(before.sum())
    rng = np.random.default_rng(23)
    d = rng.standard_normal((1500, 3))
    gpu_ctx.scan_upload(2.2 * d / np.linalg.norm(d, axis=1, keepdims=True), scan_covs(1500))
    gone, cs = gpu_ctx.map_carve_resident(np.eye(4), dict(max_range=10.0))
    assert cs.removed > 20
    gpu_ctx.scan_upload(pts[:1500], covs[:1500])
    for level in (0, 2):
        check(gpu_ctx, POSES, level, (2, 2, 1), 1, ("carved", level))


def test_a_grown_table_an_insertion_and_a_call_with_nothing_changed(gpu_ctx):
    first, second = random_keys(300, 5, seed=31), random_keys(3000, 10, seed=32)
    pts, covs = fill(gpu_ctx, first, np.ones(len(first), dtype=np.int64), 1000, hint=0)
    gpu_ctx.scan_upload(pts, covs)
    slots = gpu_ctx.map_levels_build(3).slots[0]
    a = gpu_ctx.locate_resident(POSES, 2, (3, 3, 1))
    assert a.launches == 2
    fill(gpu_ctx, second, np.full(len(second), 2), 1000, seed=33, reset=False)
    assert gpu_ctx.map_size()[1] > slots          # grown and rehashed
    b = gpu_ctx.locate_resident(POSES, 2, (3, 3, 1))          # no explicit build: the call rebuilds the three levels
    assert b.launches == 2 + 6 and int(b.hits.sum()) > int(a.hits.sum())
    c, _ = check(gpu_ctx, POSES, 2, (3, 3, 1), 1, "grown")
    assert c.launches == 2 and np.array_equal(c.hits, b.hits)          # nothing changed: no level build
    check(gpu_ctx, POSES, 0, (3, 3, 1), 1, "grown, the map itself")


# ---- cross-checks against existing entries ------------------------------------------------------------------------------
def test_a_window_of_one_cell_counts_what_evaluate_and_round_0_of_a_level_stage_count(gpu_ctx, lidar):
    load_lidar(gpu_ctx, lidar, 1500)
    poses = [np.eye(4), yaw(2.0, (0.1, -0.05, 0.02)), tilted()]
    ev = gpu_ctx.evaluate_resident(poses)
    got = gpu_ctx.locate_resident(poses, 0, (0, 0, 0))
    assert [int(h) for h in got.hits[:, 0]] == [e.correspondences for e in ev] and got.hits[0, 0] > 100
    one = dict(max_iteration=1, translation_sq_threshold=1e-12, cosine_threshold=1.0 - 1e-12)
    for level in range(4):
        for j, T in enumerate(poses[:2]):
            _, stages = gpu_ctx.align_resident_levels(T, [level], one, allow_degenerate=True)
            hits = gpu_ctx.locate_resident(T, level, (0, 0, 0)).hits
            assert int(stages[0].corr_count[0]) == int(hits[0, 0]), (level, j)


# ---- read-only ----------------------------------------------------------------------------------------------------------
def test_the_call_changes_nothing(lidar):
    from eskf_lio_amd import capi
    with capi.Context(0) as ctx:
        load_lidar(ctx, lidar, 1000, levels=2)
        guess = yaw(0.5, (0.05, -0.03, 0.02))
        first = ctx.align_resident(guess, 4, 1e-12, 1.0 - 1e-12, allow_degenerate=True)
        before, generation, size = ctx.map_export(), ctx.counter(COUNTER_SCAN_GENERATION), ctx.map_size()
        a = ctx.locate_resident(POSES, 2, (3, 3, 1), 2)
        b = ctx.locate_resident(POSES, 0, (1, 1, 1))
        assert a.hits.any() and b.hits.any()
        after = ctx.map_export()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after)) and ctx.map_size() == size
        assert ctx.counter(COUNTER_SCAN_GENERATION) == generation
        second = ctx.align_resident(guess, 4, 1e-12, 1.0 - 1e-12, allow_degenerate=True)
        assert first.pose.tobytes() == second.pose.tobytes() and first.iterations == second.iterations
        assert first.normal_eq.tobytes() == second.normal_eq.tobytes() and np.array_equal(first.corr_count, second.corr_count)
        assert np.array_equal(ctx.locate_resident(POSES, 2, (3, 3, 1), 2).hits, a.hits)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_come_in_the_headers_order_with_their_texts(gpu_ctx, lidar):
    from eskf_lio_amd import capi
    lib = capi.load_library()
    h = gpu_ctx._h
    dp = C.POINTER(C.c_double)
    good = np.ascontiguousarray(np.stack([capi.pose_to_abi(np.eye(4))] * 2))
    bad = good.copy()
    bad[1, 13] = np.inf
    best = (capi.LocateBest * 64)()
    C.memset(best, 0xA5, C.sizeof(best))
    untouched = bytes(best)
    plane = np.full(4096, 7, dtype=np.uint32)
    stats = capi.LocateStats()
    C.memset(C.byref(stats), 0xA5, C.sizeof(stats))
    stats_before = bytes(stats)

    def call(poses=good, k=2, level=0, window=(1, 1, 1), stride=1, params=True, out=best):
        p = capi.LocateParams(level, (C.c_int32 * 3)(*window), stride)
        return lib.vgicp_locate_resident(h, poses.ctypes.data_as(dp) if poses is not None else None, k,
                                         C.byref(p) if params else None, out, plane.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         C.byref(stats))

    def refused(rc, status, text):
        assert rc == status and text in gpu_ctx.last_error(), (rc, gpu_ctx.last_error())

    # everything is wrong at once on a context with no map, no scan and no level: the rules answer one after the other
    wrong = dict(poses=bad, k=65, level=5, window=(33, 0, 0), stride=0)
    refused(call(**dict(wrong, poses=None)), capi.ERR_BAD_ARGUMENT, "NULL pointer")                                      # 1
    refused(call(**dict(wrong, params=False)), capi.ERR_BAD_ARGUMENT, "NULL pointer")
    refused(call(**dict(wrong, out=None)), capi.ERR_BAD_ARGUMENT, "NULL pointer")
    refused(call(**wrong), capi.ERR_BAD_ARGUMENT, "k must be 1 ..")                                                      # 2
    refused(call(**dict(wrong, k=0)), capi.ERR_BAD_ARGUMENT, "k must be 1 ..")
    refused(call(**dict(wrong, k=2)), capi.ERR_BAD_ARGUMENT, "level must be 0 ..")
    refused(call(**dict(wrong, k=2, level=-1)), capi.ERR_BAD_ARGUMENT, "level must be 0 ..")
    refused(call(**dict(wrong, k=2, level=2)), capi.ERR_BAD_ARGUMENT, "a half-width of the window")
    refused(call(**dict(wrong, k=2, level=2, window=(0, -1, 0))), capi.ERR_BAD_ARGUMENT, "a half-width of the window")
    refused(call(**dict(wrong, k=2, level=2, window=(10, 10, 5))), capi.ERR_BAD_ARGUMENT, "more than VGICP_LOCATE_MAX_CELLS")
    refused(call(poses=bad, level=2, stride=0), capi.ERR_BAD_ARGUMENT, "stride must be >= 1")
    refused(call(poses=bad, level=2), capi.ERR_NOT_READY, "above the number of levels asked for")                         # 3
    refused(call(poses=bad), capi.ERR_BAD_ARGUMENT, "an entry of a pose is not finite")                                  # 4
    refused(call(), capi.ERR_NOT_READY, "no voxel map")                                                                  # 6
    gpu_ctx.map_reset(VOXEL, 100)
    refused(call(), capi.ERR_NOT_READY, "no scan resident")
    assert call(poses=bad, k=1) == capi.ERR_NOT_READY          # the second pose is not read with k == 1
    # 5: a multi-device context, with the sentence of the other resident calls, in front of rule 6 (it has no map)
    with capi.Context([0, 0]) as multi:
        p = capi.LocateParams(0, (C.c_int32 * 3)(1, 1, 1), 1)
        rc = lib.vgicp_locate_resident(multi._h, good.ctypes.data_as(dp), 2, C.byref(p), best, None, C.byref(stats))
        assert rc == capi.ERR_BAD_ARGUMENT
        assert "not available on multi-device contexts, communicators and peer-connected contexts" in multi.last_error()
    assert bytes(best) == untouched and bytes(stats) == stats_before and np.all(plane == 7)
    load_lidar(gpu_ctx, lidar, 63, levels=0)
    assert call() == capi.OK and bytes(best) != untouched and bytes(stats) != stats_before


# ---- the point of it ----------------------------------------------------------------------------------------------------
def test_the_pipeline_on_the_device_from_a_guess_metres_and_tens_of_degrees_off(gpu_ctx, oracle):
    """Locate on a 64-yaw fan at level 3, the chain 3 -> 2 -> 1 -> 0 from the four best poses, the winner by the evaluation's
    correspondences: the restatement's ranking and hits exactly, the oracle's chain round for round, the winner where the
    plain align from the identity ends."""
    mp, mc, sp, sc = ml.recipe(oracle)
    omap = oracle.OracleMap(VOXEL, ml.CAP)
    omap.insert(mp, mc)
    levels = ml.levels_of(*omap.export(), 3)
    maps = [omap] + [ml.oracle_level_map(oracle, levels[l], VOXEL * 2 ** l) for l in (1, 2, 3)]
    star = omap.align(sp, sc, np.eye(4), ml.FINE["max_iteration"], ml.FINE["translation_sq_threshold"], ml.FINE["cosine_threshold"]).pose
    gpu_ctx.map_reset(VOXEL, 16000)
    gpu_ctx.map_insert_scan(mp, mc, np.eye(4), ml.CAP)
    gpu_ctx.scan_upload(sp, sc)
    gpu_ctx.map_levels_build(3)
    guess = lo.wrong_guess(*lo.WRONG_GUESSES[0])
    fan = lo.yaw_fan(guess, lo.YAWS)
    got, want = check(gpu_ctx, fan, lo.LEVEL, lo.WINDOW, 1, "pipeline")
    order = lo.ranking(got.best)
    assert order == lo.ranking(want)
    params = [ml.COARSE] * (len(ml.SCHEDULE) - 1) + [ml.FINE]
    ends = []
    for j in order[:lo.KEEP]:
        pose, stages = gpu_ctx.align_resident_levels(got.best[j]["pose"], ml.SCHEDULE, params, allow_degenerate=True)
        ref_pose, ref = ml.oracle_chain(oracle, maps, sp, sc, want[j].pose)
        assert [s.iterations for s in stages] == [r.iterations for r in ref], (j, [s.iterations for s in stages])
        ends.append((gpu_ctx.evaluate_resident([pose])[0], pose, j))
    ev, pose, j = max(ends, key=lambda e: (e[0].correspondences, -e[0].cost))
    near = ml.distance(pose, star)
    print(f"winner: pose {j} of the fan, offset {got.best[j]['offset']}, {got.best[j]['hits']} hits, {ev.correspondences} matches, "
          f"{1e3 * near:.3f} mm from P* ({pose_error(pose, star)[1]:.2e} rad); locate device {1e6 * got.device_seconds:.1f} us")
    assert near <= ml.NEAR_LIMIT
