"""The map's coarser levels on the device (include/vgicp_hip_map_levels.h): vgicp_map_levels_build, vgicp_map_level_size,
vgicp_map_level_export and vgicp_align_resident_levels.

Every level is compared bit for bit with the numpy restatement of the rule (tests/map_levels_reference.py, checked on its
own by tests/test_map_levels_cpu.py) applied to the map the device itself exports; a stage of the align is compared bit
for bit with vgicp_align_resident on a second context whose MAP is the exported level; the chain is compared with the
oracle's chain on the recipe of the coarse-to-fine experiment."""
import ctypes as C
import os

import numpy as np
import pytest

import map_levels_reference as ml
from conftest import POSE_TOL_M, POSE_TOL_RAD, TIGHT_POSE_TOL, pose_error
from test_voxel_table import voxel_hash

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = ml.VOXEL
LEVELS = ml.LEVELS_MAX


# ---- maps -------------------------------------------------------------------------------------------------------------
def points_in(keys, per_voxel, seed):
    """per_voxel[i] points inside voxel keys[i] (a tenth of a voxel away from its faces), shuffled, with covariances."""
    from eskf_lio_amd import synth
    rng = np.random.default_rng(seed)
    k = np.repeat(np.asarray(keys, dtype=np.int64), np.asarray(per_voxel, dtype=np.int64), axis=0)
    pts = (k.astype(np.float64) + rng.uniform(0.1, 0.9, size=k.shape)) * VOXEL
    pts = pts[rng.permutation(len(pts))]
    covs = synth.disc_covariances(seed + 1, 16, np.arange(len(pts), dtype=np.uint64))
    return pts, covs


def random_keys(n, span, seed):
    rng = np.random.default_rng(seed)
    return np.unique(rng.integers(-span, span, size=(n, 3)), axis=0).astype(np.int32)


def fill(ctx, keys, per_voxel, cap, seed=3, hint=None, reset=True):
    pts, covs = points_in(keys, per_voxel, seed)
    if reset:
        ctx.map_reset(VOXEL, len(keys) if hint is None else hint)
    if len(pts):
        ctx.map_insert_scan(pts, covs, np.eye(4), cap)
    return pts, covs


def device_levels(ctx, levels=LEVELS):
    return [ml.as_level(*ctx.map_level_export(l)) for l in range(levels + 1)]


def assert_levels_are_the_rule(ctx, levels=LEVELS, what=""):
    """Levels 1 .. `levels` of the context against the restatement applied to the map the context exports."""
    want = ml.levels_of(*ctx.map_export(), levels)
    got = device_levels(ctx, levels)
    for l in range(levels + 1):
        assert len(got[l]) == len(want[l]) == ctx.map_level_size(l)[0], (what, l, len(got[l]), len(want[l]))
        assert np.array_equal(got[l].keys, want[l].keys), (what, l)
        assert np.array_equal(got[l].counts, want[l].counts), (what, l)
        assert got[l].means.tobytes() == want[l].means.tobytes(), (what, l)
        assert got[l].covs.tobytes() == want[l].covs.tobytes(), (what, l)
        assert ctx.map_level_size(l)[2] == VOXEL * 2 ** l
    return want


# ---- every level equals the restatement bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("cap", (1, 3, 1000))
def test_levels_of_a_map_whose_siblings_differ_in_count(gpu_ctx, cap):
    """(a) 1 951 voxels on both sides of 0 with 1 .. 6 points each: under the caps 1, 3 and 1000 the counts of siblings
    differ (and under cap 3 some are frozen there)."""
    keys = random_keys(2400, 9, seed=11)
    per = np.random.default_rng(12).integers(1, 7, size=len(keys))
    fill(gpu_ctx, keys, per, cap)
    st = gpu_ctx.map_levels_build(LEVELS)
    assert st.levels == LEVELS and st.launches == 2 * LEVELS and st.device_seconds > 0.0
    want = assert_levels_are_the_rule(gpu_ctx, what=f"cap {cap}")
    assert st.voxels == [len(lv) for lv in want] and st.voxels[0] == len(keys)
    assert all(s >= 2 * st.voxels[0] for s in st.slots[1:])          # at least half of every level's slots stay EMPTY
    counts = want[0].counts
    assert counts.max() == min(cap, 6) and (cap == 1 or len(np.unique(counts)) > 1)
    merged = sum(int(np.sum(want[l].counts > want[0].counts.max())) for l in (1, 2))
    assert merged > 100          # parents with several children
    print(f"cap {cap}: voxels {st.voxels} slots {st.slots} device {1e6 * st.device_seconds:.1f} us")


def test_all_eight_children_of_parents_that_straddle_zero(gpu_ctx):
    """(b) keys -2 .. 1 on every axis fully occupied."""
    g = np.arange(-2, 2)
    keys = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    fill(gpu_ctx, keys, np.random.default_rng(1).integers(1, 5, size=64), 1000)
    gpu_ctx.map_levels_build(LEVELS)
    want = assert_levels_are_the_rule(gpu_ctx)
    assert [len(lv) for lv in want] == [64, 8, 8, 8, 8] and want[1].counts.min() >= 8


def test_a_map_of_one_voxel_and_an_empty_map(gpu_ctx):
    """(c)"""
    fill(gpu_ctx, np.array([[-3, 5, 0]], dtype=np.int32), [4], 1000)
    gpu_ctx.map_levels_build(LEVELS)
    want = assert_levels_are_the_rule(gpu_ctx)
    assert [len(lv) for lv in want] == [1] * 5 and want[4].keys.tolist() == [[-1, 0, 0]]
    assert want[4].means.tobytes() == want[0].means.tobytes() and want[4].counts.tolist() == [4]          # the child's bits, four times
    gpu_ctx.map_reset(VOXEL, 0)
    for l in range(LEVELS + 1):          # vgicp_map_reset keeps the number of levels and empties them
        assert gpu_ctx.map_level_size(l)[0] == 0 and len(gpu_ctx.map_level_export(l)[0]) == 0
    assert gpu_ctx.map_levels_build(LEVELS).voxels == [0] * 5


@pytest.mark.parametrize("parents", (63, 64, 65, 127, 129))
def test_parent_counts_around_multiples_of_eight(gpu_ctx, parents):
    """(d) 8 k - 1, 8 k and 8 k + 1 parents at level 1, each with one to three children."""
    rng = np.random.default_rng(parents)
    pk = np.unique(rng.integers(-6, 6, size=(4 * parents, 3)), axis=0)[:parents]
    assert len(pk) == parents
    keys = []
    for k in pk:
        octs = rng.choice(8, size=rng.integers(1, 4), replace=False)
        keys += [[2 * k[0] + (o & 1), 2 * k[1] + ((o >> 1) & 1), 2 * k[2] + (o >> 2)] for o in octs]
    keys = np.array(keys, dtype=np.int32)
    fill(gpu_ctx, keys, rng.integers(1, 4, size=len(keys)), 1000)
    st = gpu_ctx.map_levels_build(LEVELS)
    assert st.voxels[1] == parents
    assert_levels_are_the_rule(gpu_ctx, what=f"{parents} parents")


def crafted_keys():
    """(e) Some 670 cells around 0, of which: a family of >= 24 whose keys collide in the FINE table (one home slot under its
    mask), and a family of >= 24 whose PARENTS collide in the level-1 table — crafted from the numpy voxel_hash."""
    fine_slots, level_slots = 4096, 2048          # vgicp_map_reset(hint 1000): 4096 slots; level tables: 2 x <= 1000 voxels
    g = np.stack(np.meshgrid(*[np.arange(-40, 40)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    home = voxel_hash(g) & np.uint32(fine_slots - 1)
    fam_fine = g[home == home[12345]][:40]
    parents = np.unique(g >> 1, axis=0).astype(np.int32)
    phome = voxel_hash(parents) & np.uint32(level_slots - 1)
    fam_parents = parents[phome == phome[777]][:30]
    rng = np.random.default_rng(4)
    kids = np.array([[2 * k[0] + rng.integers(2), 2 * k[1] + rng.integers(2), 2 * k[2] + rng.integers(2)] for k in fam_parents],
                    dtype=np.int32)
    other = g[rng.choice(len(g), 600, replace=False)]
    keys = np.unique(np.concatenate([fam_fine, kids, other]), axis=0)
    assert len(fam_fine) >= 24 and len(fam_parents) >= 24 and len(keys) <= 1000
    return keys, fam_fine, fam_parents, fine_slots, level_slots


def test_children_that_collide_in_the_fine_table_and_parents_that_collide_in_the_level_table(gpu_ctx):
    keys, fam_fine, fam_parents, fine_slots, level_slots = crafted_keys()
    fill(gpu_ctx, keys, np.random.default_rng(5).integers(1, 4, size=len(keys)), 1000, hint=1000)
    st = gpu_ctx.map_levels_build(LEVELS)
    assert st.slots[0] == fine_slots and st.slots[1] == level_slots          # the masks the families were crafted for
    assert len(np.unique(voxel_hash(fam_fine) & np.uint32(fine_slots - 1))) == 1
    assert len(np.unique(voxel_hash(fam_parents) & np.uint32(level_slots - 1))) == 1
    want = assert_levels_are_the_rule(gpu_ctx)
    have = {tuple(k) for k in want[1].keys.tolist()}
    assert all(tuple(k) in have for k in fam_parents.tolist())


def test_tombstoned_children_are_gone_from_the_sums(gpu_ctx):
    """(f) after vgicp_map_evict and after vgicp_map_carve_resident."""
    keys = random_keys(2400, 9, seed=21)
    fill(gpu_ctx, keys, np.random.default_rng(22).integers(1, 5, size=len(keys)), 1000)
    gpu_ctx.map_levels_build(3)
    before = assert_levels_are_the_rule(gpu_ctx, 3)
    removed = gpu_ctx.map_evict(np.array([1.5, 0.0, 0.0]), 1.6)
    assert 100 < removed < len(keys) - 100
    after = assert_levels_are_the_rule(gpu_ctx, 3, "evicted")          # no explicit build: the export rebuilds
    assert int(after[3].counts.sum()) < int(before[3].counts.sum()) and len(after[1]) < len(before[1])
    # carve: a scan of returns at 2.2 m seen from the origin removes what lies in front of them
    rng = np.random.default_rng(23)
    d = rng.standard_normal((1500, 3))
    pts = 2.2 * d / np.linalg.norm(d, axis=1, keepdims=True)
    gpu_ctx.scan_upload(pts, np.tile((1e-3 * np.eye(3)).reshape(9), (len(pts), 1)))
    gone, cs = gpu_ctx.map_carve_resident(np.eye(4), dict(max_range=10.0))
    assert cs.removed > 20
    carved = assert_levels_are_the_rule(gpu_ctx, 3, "carved")
    assert int(carved[3].counts.sum()) < int(after[3].counts.sum())


def test_levels_follow_a_fine_table_that_grows(gpu_ctx):
    """(g) a map made with no capacity hint grows (and rehashes) under the second insertion."""
    first, second = random_keys(300, 5, seed=31), random_keys(3000, 10, seed=32)
    fill(gpu_ctx, first, np.ones(len(first), dtype=np.int64), 1000, hint=0)
    st0 = gpu_ctx.map_levels_build(LEVELS)
    assert_levels_are_the_rule(gpu_ctx)
    fill(gpu_ctx, second, np.full(len(second), 2), 1000, seed=33, reset=False)
    assert gpu_ctx.map_size()[1] > st0.slots[0]
    assert_levels_are_the_rule(gpu_ctx, what="grown")          # lazily, into larger level tables
    st1 = gpu_ctx.map_levels_build(LEVELS)
    assert st1.launches == 0 and st1.slots[1] > st0.slots[1] and st1.voxels[0] > st0.voxels[0]


@pytest.mark.parametrize("hint", (1 << 17, 1 << 18))
def test_fine_tables_either_side_of_the_wide_claims_threshold(gpu_ctx, hint):
    """The claim launch takes four slots per thread from 2^20 slots of the finer table on (kClaimWideSlots,
    vgicp_levels.hip), one below: a map made with a capacity hint of 2^17 has 2^19 slots, one of 2^18 has 2^20.  The
    rule holds either way."""
    keys = random_keys(2400, 9, seed=61)
    fill(gpu_ctx, keys, np.random.default_rng(62).integers(1, 5, size=len(keys)), 1000, hint=hint)
    st = gpu_ctx.map_levels_build(LEVELS)
    assert st.slots[0] == 4 * hint and st.launches == 2 * LEVELS
    assert_levels_are_the_rule(gpu_ctx, what=f"{st.slots[0]} fine slots")


def test_two_builds_of_the_same_map_are_bitwise_equal(gpu_ctx):
    from eskf_lio_amd import capi
    keys = random_keys(2400, 9, seed=41)
    per = np.random.default_rng(42).integers(1, 7, size=len(keys))
    fill(gpu_ctx, keys, per, 1000)
    assert gpu_ctx.map_levels_build(LEVELS).launches == 2 * LEVELS
    a = device_levels(gpu_ctx)
    assert gpu_ctx.map_levels_build(0).launches == 0          # released ...
    assert gpu_ctx.map_levels_build(LEVELS).launches == 2 * LEVELS          # ... and built anew
    b = device_levels(gpu_ctx)
    with capi.Context(0) as other:          # ... and on another context, from the same insertion
        fill(other, keys, per, 1000)
        other.map_levels_build(LEVELS)
        c = device_levels(other)
    for l in range(LEVELS + 1):
        assert ml.same_level(a[l], b[l]) and ml.same_level(a[l], c[l]), l


# ---- laziness ---------------------------------------------------------------------------------------------------------
def test_levels_are_rebuilt_when_the_map_has_changed_and_only_then(gpu_ctx):
    keys = random_keys(1200, 7, seed=51)
    fill(gpu_ctx, keys, np.ones(len(keys), dtype=np.int64), 1000)
    assert gpu_ctx.map_levels_build(3).launches == 6
    assert gpu_ctx.map_levels_build(3).launches == 0          # nothing changed: nothing is launched
    more = random_keys(400, 9, seed=52)
    fill(gpu_ctx, more, np.ones(len(more), dtype=np.int64), 1000, seed=53, reset=False)
    gpu_ctx.frame_stats(reset=True)
    got = ml.as_level(*gpu_ctx.map_level_export(3))          # no explicit build
    # the size query and the export both read level 3: six launches of one rebuild, one of the export's own kernel
    assert gpu_ctx.frame_stats(reset=True).kernel_launches == 6 + 1
    want = ml.levels_of(*gpu_ctx.map_export(), 3)[3]
    # every point of both insertions is counted at level 3 (the two key sets overlap: some voxels hold two points)
    assert ml.same_level(got, want) and int(want.counts.sum()) == len(keys) + len(more)
    gpu_ctx.frame_stats(reset=True)
    again = ml.as_level(*gpu_ctx.map_level_export(3))
    assert gpu_ctx.frame_stats(reset=True).kernel_launches == 1          # the export's kernel alone
    assert ml.same_level(again, want) and gpu_ctx.map_levels_build(3).launches == 0
    # asking for one level more builds that level alone
    assert gpu_ctx.map_levels_build(4).launches == 2


# ---- a level align is a plain align ------------------------------------------------------------------------------------
FINE = ml.FINE
COARSE = ml.COARSE


@pytest.fixture(scope="module")
def scene(oracle):
    """The recipe of the coarse-to-fine experiment: map points, scan, and the oracle's side of it (computed once)."""
    mp, mc, sp, sc = ml.recipe(oracle)
    omap = oracle.OracleMap(VOXEL, ml.CAP)
    omap.insert(mp, mc)
    levels = ml.levels_of(*omap.export(), 3)
    maps = [omap] + [ml.oracle_level_map(oracle, levels[l], VOXEL * 2 ** l) for l in (1, 2, 3)]
    star = omap.align(sp, sc, np.eye(4), FINE["max_iteration"], FINE["translation_sq_threshold"], FINE["cosine_threshold"]).pose
    return dict(mp=mp, mc=mc, sp=sp, sc=sc, levels=levels, maps=maps, star=star)


def load_scene(ctx, scene, levels=3):
    ctx.map_reset(VOXEL, 16000)
    ctx.map_insert_scan(scene["mp"], scene["mc"], np.eye(4), ml.CAP)
    ctx.scan_upload(scene["sp"], scene["sc"])
    if levels:
        ctx.map_levels_build(levels)


def same_align(a, b):
    return (a.iterations == b.iterations and a.converged == b.converged and np.array_equal(a.corr_count, b.corr_count)
            and a.normal_eq.tobytes() == b.normal_eq.tobytes())


def prior_of(pose):
    info = np.diag([4.0, 4.0, 4.0, 9.0, 9.0, 9.0])
    return pose, info


@pytest.mark.parametrize("variant", ("plain", "no_persistent", "huber", "prior"))
def test_a_stage_is_vgicp_align_resident_over_the_exported_level(gpu_ctx, scene, variant):
    """On a second context the exported level l IS the map (vgicp_map_reset at the level's voxel size, vgicp_map_upsert):
    vgicp_align_resident there and the single stage l here return the same pose, rounds, counts and normal equations."""
    from eskf_lio_amd import capi
    load_scene(gpu_ctx, scene)
    flags = capi.FLAG_NO_PERSISTENT if variant == "no_persistent" else 0
    guess = ml.shifted(0.2)
    with capi.Context(0) as other:
        for ctx in (gpu_ctx, other):
            if variant == "huber":
                ctx.set_robust("huber", 0.1, 0.5)
            if variant == "prior":
                ctx.set_pose_prior(*prior_of(ml.shifted(0.1)))
        other.scan_upload(scene["sp"], scene["sc"])
        for l in range(4):
            keys, means, covs, _ = gpu_ctx.map_level_export(l)
            other.map_reset(VOXEL * 2 ** l, len(keys))
            other.map_upsert(keys, means, covs)
            p = COARSE if l else FINE
            want = other.align_resident(guess, p["max_iteration"], p["translation_sq_threshold"], p["cosine_threshold"], flags=flags)
            pose, (got,) = gpu_ctx.align_resident_levels(guess, [l], dict(p, flags=flags))
            assert pose.tobytes() == want.pose.tobytes(), (variant, l)
            assert same_align(got, want) and got.iterations >= 1 and got.launches == want.launches, (variant, l)
            assert got.corr_count[0] > 1000
            if l == 0:          # stage 0 is the plain call on the context itself, too
                own = gpu_ctx.align_resident(guess, p["max_iteration"], p["translation_sq_threshold"], p["cosine_threshold"], flags=flags)
                assert own.pose.tobytes() == pose.tobytes() and same_align(own, got)


def stage_params():
    return [COARSE] * 3 + [FINE]


def test_a_schedule_is_the_chain_of_its_stages(gpu_ctx, scene):
    load_scene(gpu_ctx, scene)
    guess = ml.shifted(0.9)
    pose, stages = gpu_ctx.align_resident_levels(guess, ml.SCHEDULE, stage_params())
    at = guess
    for l, p, st in zip(ml.SCHEDULE, stage_params(), stages):
        at, (single,) = gpu_ctx.align_resident_levels(at, [l], p)
        assert same_align(single, st), l
    assert at.tobytes() == pose.tobytes()
    assert [s.iterations for s in stages][-1] >= 1 and len(stages) == 4
    # the sequence of levels is free: ascending, repeated, not ending at 0
    up, st_up = gpu_ctx.align_resident_levels(guess, [1, 1, 3], COARSE)
    a, _ = gpu_ctx.align_resident_levels(guess, [1], COARSE)
    b, _ = gpu_ctx.align_resident_levels(a, [1], COARSE)
    c, _ = gpu_ctx.align_resident_levels(b, [3], COARSE)
    assert up.tobytes() == c.tobytes() and len(st_up) == 3


@pytest.mark.parametrize("dx", (0.9,))
def test_the_chain_against_the_oracles_chain_where_the_plain_align_fails(gpu_ctx, oracle, scene, dx):
    load_scene(gpu_ctx, scene)
    for l in range(4):          # the device's levels are the ones the oracle's maps were made of
        assert ml.same_level(ml.as_level(*gpu_ctx.map_level_export(l)), scene["levels"][l]), l
    guess = ml.shifted(dx)
    want_pose, want = ml.oracle_chain(oracle, scene["maps"], scene["sp"], scene["sc"], guess)
    pose, stages = gpu_ctx.align_resident_levels(guess, ml.SCHEDULE, stage_params())
    for l, got, ref in zip(ml.SCHEDULE, stages, want):
        assert got.iterations == ref.iterations and got.converged == ref.converged, l
        assert np.array_equal(got.corr_count, ref.corr_count), (l, got.corr_count, ref.corr_count)
    dt, dr = pose_error(pose, want_pose)
    plain = gpu_ctx.align_resident(guess, FINE["max_iteration"], FINE["translation_sq_threshold"], FINE["cosine_threshold"])
    far, near = ml.distance(plain.pose, scene["star"]), ml.distance(pose, scene["star"])
    print(f"shift {dx} m: chain {1e3 * near:.3f} mm from P* (oracle's chain: {dt:.2e} m {dr:.2e} rad away), plain {far:.4f} m; "
          f"device us per stage {[round(1e6 * s.device_seconds, 1) for s in stages]}, plain {1e6 * plain.device_seconds:.1f}")
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert dt <= TIGHT_POSE_TOL and dr <= TIGHT_POSE_TOL
    assert far >= ml.FAR_LIMIT and near <= ml.NEAR_LIMIT


def test_a_context_with_no_levels_aligns_as_before_and_after_a_build_and_release(gpu_ctx, scene):
    load_scene(gpu_ctx, scene, levels=0)
    guess = ml.shifted(0.1)
    args = (guess, FINE["max_iteration"], FINE["translation_sq_threshold"], FINE["cosine_threshold"])
    before = gpu_ctx.align_resident(*args)
    gpu_ctx.map_levels_build(3)
    during = gpu_ctx.align_resident(*args)
    gpu_ctx.map_levels_build(0)
    after = gpu_ctx.align_resident(*args)
    for other in (during, after):
        assert other.pose.tobytes() == before.pose.tobytes() and same_align(other, before) and other.launches == before.launches
    with pytest.raises(Exception, match="above the number of levels"):
        gpu_ctx.map_level_size(1)


# ---- the Python chain -------------------------------------------------------------------------------------------------
def test_replay_with_levels_ends_where_the_abi_chain_driven_from_python_ends(tmp_path):
    """tools/replay.py --resident --levels 3,2,1,0 (DeviceBackend over the capi.py wrappers) against the same frame loop
    whose align calls vgicp_align_resident_levels through ctypes itself, stage by stage: the same poses, bit for bit."""
    import importlib.util
    from eskf_lio_amd import capi, replay, synth
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = ["--synthetic", "4", "--points", "6000", "--resident", "--levels", "3,2,1,0", "--coarse-max-iteration", "20"]
    summary = tool.main(args + ["--out", str(tmp_path / "levels.tum")])
    assert summary["poses"] == 4

    cfg = tool.coarse_to_fine_config(replay.DEFAULT_CONFIG, tool.parse_args(args))
    levels, coarse = replay.coarse_to_fine_of(cfg)
    assert levels == [3, 2, 1, 0] and coarse == dict(max_iteration=20, translation_sq_threshold=1e-4, cosine_threshold=0.999)
    reg = cfg["registration"]
    rounds = []

    class AbiChain(replay.DeviceBackend):
        def _align(self, guess):
            lib, dp = capi.load_library(), C.POINTER(C.c_double)
            at = capi.pose_to_abi(guess)
            for i, l in enumerate(levels):
                p = capi.Params(coarse["max_iteration"], 0, coarse["translation_sq_threshold"], coarse["cosine_threshold"], 0, 0) \
                    if i + 1 < len(levels) else \
                    capi.Params(reg["max_iteration"], 0, reg["translation_sq_threshold"], reg["cosine_threshold"], 0, 0)
                st, out = capi.Stats(), np.zeros(16)
                rc = lib.vgicp_align_resident_levels(self.ctx._h, at.ctypes.data_as(dp), 1, (C.c_int32 * 1)(l), C.byref(p),
                                                     out.ctypes.data_as(dp), C.byref(st))
                assert rc == capi.OK, self.ctx.last_error()
                rounds.append(st.iterations)
                at = out
            return capi.pose_from_abi(at), st

    raw, _ = synth.make_sensor_stream(frames=4, points_per_frame=6000, world_points=60_000)
    events = [(a, replay.ImuMeasurement(e[1], e[2], e[3]) if e[0] == "imu" else replay.LidarMeasurement(e[1], e[2])) for a, e in raw]
    traj = replay.Odometry(cfg, AbiChain(cfg)).run(events)
    assert len(traj) == len(summary["trajectory"]) == 4 and len(rounds) == 3 * 4 and min(rounds) >= 1
    for (ta, A), (tb, B) in zip(traj, summary["trajectory"]):
        assert ta == tb and np.asarray(A).tobytes() == np.asarray(B).tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_come_in_the_headers_order_with_their_texts(gpu_ctx, scene):
    from eskf_lio_amd import capi
    lib = capi.load_library()
    h = gpu_ctx._h
    dp = C.POINTER(C.c_double)
    good = capi.pose_to_abi(np.eye(4))
    bad = good.copy()
    bad[13] = np.nan
    out = np.full(16, 7.0)
    ok_p = (capi.Params * 2)(capi.Params(10, 0, 1e-6, 0.9999, 0, 0), capi.Params(10, 0, 1e-6, 0.9999, 0, 0))
    neg_p = (capi.Params * 2)(capi.Params(10, 0, 1e-6, 0.9999, 0, 0), capi.Params(-1, 0, 1e-6, 0.9999, 0, 0))
    lv = lambda *v: (C.c_int32 * len(v))(*v)

    def align(guess=good, stages=2, levels=lv(0, 0), params=ok_p, pose=out):
        return lib.vgicp_align_resident_levels(h, guess.ctypes.data_as(dp) if guess is not None else None, stages, levels, params,
                                               pose.ctypes.data_as(dp) if pose is not None else None, None)

    def refused(rc, status, text):
        assert rc == status and text in gpu_ctx.last_error(), (rc, gpu_ctx.last_error())

    # everything is wrong at once on a context with no map, no scan and no level: the rules answer one after the other
    refused(align(guess=None, stages=0, levels=lv(5, 0), params=neg_p), capi.ERR_BAD_ARGUMENT, "NULL pointer")                 # 1
    refused(align(guess=bad, stages=0, levels=lv(5, 0), params=neg_p), capi.ERR_BAD_ARGUMENT, "stages must be 1 ..")           # 2
    refused(align(guess=bad, stages=9, levels=lv(5, 0), params=neg_p), capi.ERR_BAD_ARGUMENT, "stages must be 1 ..")
    refused(align(guess=bad, levels=lv(5, 0), params=neg_p), capi.ERR_BAD_ARGUMENT, "a stage's level must be 0 ..")
    refused(align(guess=bad, levels=lv(0, -1), params=neg_p), capi.ERR_BAD_ARGUMENT, "a stage's level must be 0 ..")
    refused(align(guess=bad, levels=lv(0, 2), params=neg_p), capi.ERR_NOT_READY, "above the number of levels asked for")          # 3
    refused(align(guess=bad, params=neg_p), capi.ERR_BAD_ARGUMENT, "an entry of guess is not finite")                          # 4
    refused(align(params=neg_p), capi.ERR_BAD_ARGUMENT, "stage 1: max_iteration < 0")                                         # 5
    refused(align(), capi.ERR_NOT_READY, "no voxel map")                                                                      # 7
    gpu_ctx.map_reset(VOXEL, 100)
    refused(align(), capi.ERR_NOT_READY, "no scan resident")
    assert np.all(out == 7.0)
    # the other three entries
    st = capi.LevelsStats()
    w = C.c_size_t(7)
    refused(lib.vgicp_map_levels_build(h, 5, C.byref(st)), capi.ERR_BAD_ARGUMENT, "levels must be 0 ..")
    refused(lib.vgicp_map_levels_build(h, -1, None), capi.ERR_BAD_ARGUMENT, "levels must be 0 ..")
    refused(lib.vgicp_map_level_size(h, 5, None, None, None), capi.ERR_BAD_ARGUMENT, "level must be 0 ..")
    refused(lib.vgicp_map_level_size(h, 1, None, None, None), capi.ERR_NOT_READY, "above the number of levels asked for")
    refused(lib.vgicp_map_level_export(h, 0, 0, None, None, None, None, None), capi.ERR_BAD_ARGUMENT, "written is NULL")
    refused(lib.vgicp_map_level_export(h, 2, 0, None, None, None, None, C.byref(w)), capi.ERR_NOT_READY, "above the number of levels")
    assert w.value == 7 and lib.vgicp_map_level_size(h, 0, None, None, None) == capi.OK
    load_scene(gpu_ctx, scene, levels=1)
    refused(lib.vgicp_map_level_export(h, 1, 10, None, None, None, None, C.byref(w)), capi.ERR_BAD_ARGUMENT, "NULL array pointer")   # 8
    assert lib.vgicp_map_level_export(h, 1, 0, None, None, None, None, C.byref(w)) == capi.OK and w.value == 0
    # 6: a multi-device context, with the sentence of the other resident calls — in front of rule 7 (it has no map)
    with capi.Context([0, 0]) as multi:
        mh = multi._h
        rc = lib.vgicp_align_resident_levels(mh, good.ctypes.data_as(dp), 2, lv(0, 0), ok_p, out.ctypes.data_as(dp), None)
        text = multi.last_error()
        assert rc == capi.ERR_BAD_ARGUMENT and "not available on multi-device contexts, communicators and peer-connected contexts" in text
        assert lib.vgicp_map_levels_build(mh, 2, None) == capi.ERR_BAD_ARGUMENT and "multi-device" in multi.last_error()
        assert lib.vgicp_map_level_size(mh, 0, None, None, None) == capi.ERR_BAD_ARGUMENT
    assert np.all(out == 7.0)
