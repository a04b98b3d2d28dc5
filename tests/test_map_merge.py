"""Map merge on the device (include/vgicp_hip_map_merge.h): vgicp_map_merge.

The destination's export after every call is compared with == against the numpy restatement of the rule
(tests/map_merge_reference.py, checked on its own and pinned against the oracle's insertion by
tests/test_map_merge_cpu.py), applied to the destination's export before the call and to the contributors in the source's
slot order.  That order is the one thing the export does not tell (the table puts colliding keys where the claims' race
puts them), so the contributors are taken from vgicp_scan_from_map into a third context, which emits them in slot order
and whose content the submap tests hold against its own rule."""
import ctypes as C
import math

import numpy as np
import pytest

import map_levels_reference as ml
import map_merge_reference as mm
import map_submap_reference as ms
from eskf_lio_amd import capi, synth
from test_map_submap import (COUNTER_SCAN_GENERATION, VOXEL, collision_free, counted_map, frame_of, payload, random_keys,
                             upsert_map)
from map_walk_reference import table_growth
from test_voxel_table import next_pow2

pytestmark = pytest.mark.gpu

INF = math.inf
ZERO = (0.0, 0.0, 0.0)


def cube(lo, hi, take=None, seed=0):
    keys = np.stack(np.meshgrid(*[np.arange(lo, hi)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    keys = keys[np.random.default_rng(seed).permutation(len(keys))]
    return keys if take is None else keys[:take]


def contributors(third, src, center=ZERO, radius=INF, frame=None, min_count=0):
    """The moved contributors in the source's slot order, and the from-map call's stats."""
    st = third.scan_from_map(src, center, radius, frame, min_count=min_count)
    if st.points == 0:
        return np.zeros((0, 3)), np.zeros((0, 9)), np.zeros(0, dtype=np.uint64), st
    pts, covs = third.scan_download()
    _, counts = third.scan_from_map_keys()
    assert len(pts) == len(covs) == len(counts) == st.points
    return pts, covs, counts, st


def merged_reference(dst, src, third, center=ZERO, radius=INF, frame=None, min_count=0, max_count=0):
    pts, covs, counts, sub = contributors(third, src, center, radius, frame, min_count)
    return mm.merge(dst.map_export(), pts, covs, counts, VOXEL, max_count), sub


def assert_is_the_rule(dst, st, want, sub, what=""):
    assert (st.voxels, st.selected, st.too_far, st.too_few) == (sub.voxels, sub.points, sub.too_far, sub.too_few), (what, st)
    assert (st.created, st.updated, st.frozen, st.points) == (want.created, want.updated, want.frozen, want.points), (what, st, want.created,
                                                                                                                   want.updated, want.frozen, want.points)
    got = dst.map_export()
    assert len(got[0]) == len(want.keys) == dst.map_size()[0], what
    assert mm.exports_equal(got, want.export()), what          # ==, counts included


def checkpoint_bytes(ctx):
    return ctx.map_checkpoint().tobytes()


@pytest.fixture()
def three(gpu_ctx):
    src, third = capi.Context(0), capi.Context(0)
    yield gpu_ctx, src, third
    src.close()
    third.close()


# ---- 1. copy into an empty map -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 257, 2000))
def test_the_identity_into_an_empty_map_is_a_copy(three, n):
    dst, src, _ = three
    counted_map(src, random_keys(n, 2 if n == 1 else 8, seed=n))
    dst.map_reset(VOXEL, n)
    st = dst.map_merge(src)
    assert mm.exports_equal(dst.map_export(), src.map_export())          # by key, ==, counts included
    assert (st.created, st.updated, st.frozen, st.voxels, st.selected) == (n, 0, 0, n, n)
    assert st.points == int(src.map_export()[3].sum()) and st.launches >= 5 and st.device_seconds > 0.0
    print(f"n {n}: launches {st.launches} device {1e6 * st.device_seconds:.1f} us wall {1e6 * st.seconds:.1f} us")


def test_an_empty_source_changes_nothing_and_launches_nothing(three):
    dst, src, _ = three
    upsert_map(dst, random_keys(300, 4, seed=3))
    src.map_reset(VOXEL, 0)
    before = checkpoint_bytes(dst)
    st = dst.map_merge(src, frame=frame_of())
    assert (st.voxels, st.selected, st.created, st.updated, st.frozen, st.points, st.launches) == (0, 0, 0, 0, 0, 0, 0)
    assert checkpoint_bytes(dst) == before


# ---- 2. the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_count", (0, 4))
def test_the_rule_on_overlapping_maps_under_a_rotation(three, max_count):
    dst, src, third = three
    counted_map(dst, cube(-4, 5, seed=1), seed=11)                     # 729 voxels, counts 1 .. 5
    counted_map(src, cube(-6, 7, take=2000, seed=2), seed=12)          # 2 000 of 2 197, dense: moved voxels share destinations
    frame = frame_of(30.0, -10.0, (1.25, -0.5, 0.75))
    want, sub = merged_reference(dst, src, third, frame=frame, max_count=max_count)
    # the condition, on the reference's own grouping
    groups = list(want.groups.values())
    assert sum(1 for _, k in groups if k >= 3) >= 20
    assert sum(1 for existed, k in groups if existed and k >= 1) >= 50
    assert sum(1 for existed, _ in groups if not existed) >= 50
    assert (want.frozen > 0) == (max_count != 0)
    st = dst.map_merge(src, frame=frame, max_count=max_count)
    assert_is_the_rule(dst, st, want, sub, what=f"max_count {max_count}")
    assert st.selected == 2000 and st.points + 0 == int(want.points)
    assert int(dst.map_export()[3].sum()) == int(want.counts.sum())


# ---- 3. equals the insertion when every count is one ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_count", (1, 3, 1000))
def test_a_source_of_single_points_merges_to_what_the_insertion_leaves(three, max_count):
    dst, src, other = three
    upsert_map(src, cube(-6, 7, take=2000, seed=4), seed=21)           # every count 1
    for ctx in (dst, other):
        counted_map(ctx, cube(-4, 5, seed=5), seed=22)
    assert mm.exports_equal(dst.map_export(), other.map_export())
    frame = frame_of(30.0, -10.0, (1.25, -0.5, 0.75))
    st = dst.map_merge(src, frame=frame, max_count=max_count)
    sub = other.scan_from_map(src, ZERO, INF, frame)
    new_voxels = other.map_insert_resident(np.eye(4), max_count)
    assert sub.points == st.selected == 2000 and st.created == new_voxels > 50
    assert mm.exports_equal(dst.map_export(), other.map_export())
    assert st.frozen + st.points == 2000 and (st.frozen > 0) == (max_count < 1000)


# ---- 4. selection -------------------------------------------------------------------------------------------------------------
def test_the_radius_and_the_least_count_leave_voxels_out(three):
    dst, src, third = three
    counted_map(src, cube(-7, 7, take=2000, seed=6), seed=31)
    upsert_map(dst, cube(-3, 3, seed=7), seed=32)
    center, radius, frame = (0.25, 0.25, 0.25), 2.5, frame_of(12.0, 3.0, (0.0, 1.0, 0.0))
    want, sub = merged_reference(dst, src, third, center, radius, frame, min_count=3)
    assert sub.too_far > 100 and sub.too_few > 20 and sub.points > 50
    st = dst.map_merge(src, center, radius, frame, min_count=3)
    assert_is_the_rule(dst, st, want, sub, what="selection")
    assert st.voxels == 2000 == st.selected + st.too_far + st.too_few
    # what was left out contributed nothing: the accepted points are the selected voxels' counts alone
    keys, _, _, counts = src.map_export()
    take = ~ms.too_far(keys, VOXEL, center, radius) & (counts >= 3)
    assert int(take.sum()) == st.selected and int(counts[take].sum()) == st.points


# ---- 5. growth ----------------------------------------------------------------------------------------------------------------
def test_the_destination_grows_by_the_insertions_rule(three):
    dst, src, third = three
    counted_map(src, cube(-6, 7, take=2000, seed=8), seed=41)
    keys = cube(-2, 3, take=100, seed=9)
    upsert_map(dst, keys, seed=42, hint=16)
    assert dst.map_size() == (100, 1024)
    frame = frame_of(-20.0, 5.0, (0.5, 0.25, -0.25))
    want, sub = merged_reference(dst, src, third, frame=frame)
    st = dst.map_merge(src, frame=frame)
    assert_is_the_rule(dst, st, want, sub, what="growth")
    # plan_table_growth as the map walks model it (tests/map_walk_reference.py): (100 + 0 + 2 000) * 2 > 1 024, so a table
    # for 100 + 2 000 voxels at load 1/4
    grows, slots, _ = table_growth(1024, 100, 0, 2000)
    assert grows and dst.map_size()[1] == slots == 16384


# ---- 6. tombstones ------------------------------------------------------------------------------------------------------------
def test_tombstones_are_passed_over_and_kept(three):
    dst, src, _ = three
    keys = cube(-5, 5, seed=10)
    upsert_map(dst, keys, seed=51, hint=4000)
    slots = dst.map_size()[1]
    before = {tuple(k): (m, c) for k, m, c, _ in zip(*dst.map_export())}
    removed = dst.map_evict((0.25, 0.25, 0.25), 1.8)
    gone = keys[ms.too_far(keys, VOXEL, (0.25, 0.25, 0.25), 1.8)]
    assert removed == len(gone) > 300 and capi.map_checkpoint_info(dst.map_checkpoint())["tombstones"] == removed
    counted_map(src, gone[:250], seed=52)                               # onto the evicted keys
    st = dst.map_merge(src)
    assert (st.created, st.updated, st.selected) == (250, 0, 250) and dst.map_size() == (1000 - removed + 250, slots)
    info = capi.map_checkpoint_info(dst.map_checkpoint())
    assert info["tombstones"] == removed and info["voxels"] == 1000 - removed + 250          # no tombstone was claimed
    got = {tuple(k): (m, c, n) for k, m, c, n in zip(*dst.map_export())}
    for k, m, c, n in zip(*src.map_export()):                            # fresh: the source's bits and counts, not the evicted record's
        gm, gc, gn = got[tuple(k)]
        assert np.array_equal(gm, m) and np.array_equal(gc, c) and gn == n
        assert not np.array_equal(gm, before[tuple(k)][0])


# ---- 7. consumers of the merged map -----------------------------------------------------------------------------------------------
def test_levels_checkpoint_and_align_read_the_merged_map(three):
    dst, src, restored = three
    counted_map(dst, cube(-4, 5, seed=11), seed=61)
    counted_map(src, cube(-6, 7, take=2000, seed=12), seed=62)
    dst.map_levels_build(2)                                             # built before the merge: rebuilt lazily after it
    dst.map_merge(src, frame=frame_of(8.0, -4.0, (0.5, 0.5, 0.0)))
    want = ml.levels_of(*dst.map_export(), 2)
    for level in (1, 2):
        assert ml.same_level(ml.as_level(*dst.map_level_export(level)), want[level]), level
    blob = dst.map_checkpoint()
    restored.map_restore(blob)
    assert mm.exports_equal(restored.map_export(), dst.map_export())
    keys = dst.map_export()[0][::3]
    means, covs = payload(keys, 63)
    guess = frame_of(0.5, 0.2, (0.03, -0.02, 0.01))
    results = []
    for ctx in (dst, restored):
        ctx.scan_upload(means, covs)
        results.append(ctx.align_resident(guess, 10, 1e-6, 2.0, allow_degenerate=True))
    a, b = results
    assert a.iterations == b.iterations >= 1 and np.array_equal(a.pose, b.pose)
    assert np.array_equal(a.corr_count, b.corr_count) and np.array_equal(a.normal_eq, b.normal_eq) and a.corr_count[0] > 300


# ---- 8. untouched state and refusals -------------------------------------------------------------------------------------------
def test_the_source_and_the_destinations_scan_are_untouched_and_refusals_change_nothing(three):
    lib = capi.load_library()
    dst, src, other = three
    dst.map_reset(VOXEL, 4000)                                         # room for the source: the call itself synchronises once
    counted = cube(-4, 5, seed=13)
    means, covs = payload(counted, 72)
    dst.map_upsert(counted, means, covs)
    counted_map(src, cube(-6, 7, take=2000, seed=14), seed=73)
    for ctx, seed in ((dst, 74), (src, 75)):
        m, c = payload(counted[:200], seed)
        ctx.scan_upload(m, c)
    src_bytes, src_generation, src_scan = checkpoint_bytes(src), src.counter(COUNTER_SCAN_GENERATION), src.scan_download()
    dst_generation, dst_scan = dst.counter(COUNTER_SCAN_GENERATION), dst.scan_download()
    dst.frame_stats(reset=True)
    st = dst.map_merge(src, frame=frame_of())
    fs = dst.frame_stats(reset=True)
    assert fs.host_syncs == 1 and fs.kernel_launches == st.launches and st.created > 100 and st.updated > 100
    assert checkpoint_bytes(src) == src_bytes and src.counter(COUNTER_SCAN_GENERATION) == src_generation
    assert dst.counter(COUNTER_SCAN_GENERATION) == dst_generation
    for before, ctx in ((src_scan, src), (dst_scan, dst)):
        again = ctx.scan_download()
        assert again[0].tobytes() == before[0].tobytes() and again[1].tobytes() == before[1].tobytes()
    # refusals 4 .. 11 but rule 5 (two devices: a box with one GPU cannot make the case; tests/native/merge_plan.cpp
    # enumerates it): every case breaks the rule named and every later one it can
    empty, quarter, raw = capi.Context(0), other, capi.Context(0)
    try:
        raw.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
        raw.map_reset(VOXEL, 100)
        raw.map_insert_scan(*payload(counted[:50], 76), np.eye(4), 5)
        quarter.map_reset(VOXEL / 2, 100)
        quarter.map_upsert(counted[:50], *payload(counted[:50], 77))
        dst_bytes, raw_bytes = checkpoint_bytes(dst), checkpoint_bytes(raw)

        def call(d, s, center=ZERO, radius=1.0, frame=None, reserved=0):
            p = capi.MergeParams((C.c_double * 3)(*center), radius, (C.c_double * 16)(*capi.pose_to_abi(np.eye(4) if frame is None else frame)),
                                 0, 0, reserved)
            out = capi.MergeStats()
            C.memset(C.byref(out), 0xA5, C.sizeof(out))
            rc = lib.vgicp_map_merge(d._h if d else None, s._h if s else None, C.byref(p), C.byref(out))
            assert rc == capi.OK or bytes(out) == b"\xa5" * C.sizeof(out)          # a refused call writes no stats
            return rc, (d.last_error() if d else "")

        nan, nan_frame = float("nan"), np.eye(4)
        nan_frame[1, 3] = np.nan
        cases = (
            (4, (dst, dst, dict(reserved=1, radius=nan)), capi.ERR_BAD_ARGUMENT, "the same context"),
            (6, (dst, empty, dict(reserved=1, radius=nan, frame=nan_frame)), capi.ERR_BAD_ARGUMENT, "reserved must be 0"),
            (7, (dst, empty, dict(center=(0.0, INF, 0.0), radius=-1.0)), capi.ERR_BAD_ARGUMENT, "center or frame is not finite"),
            (7, (dst, empty, dict(frame=nan_frame, radius=nan)), capi.ERR_BAD_ARGUMENT, "center or frame is not finite"),
            (8, (dst, empty, dict(radius=nan)), capi.ERR_BAD_ARGUMENT, "radius must be >= 0"),
            (8, (dst, empty, dict(radius=-0.5)), capi.ERR_BAD_ARGUMENT, "radius must be >= 0"),
            (8, (dst, empty, dict(radius=-INF)), capi.ERR_BAD_ARGUMENT, "radius must be >= 0"),
            (9, (dst, empty, dict()), capi.ERR_NOT_READY, "no voxel map"),
            (9, (empty, quarter, dict()), capi.ERR_NOT_READY, "no voxel map"),
            (10, (dst, quarter, dict()), capi.ERR_BAD_ARGUMENT, "voxel sizes of dst and src differ"),
            (10, (raw, quarter, dict()), capi.ERR_BAD_ARGUMENT, "voxel sizes of dst and src differ"),
            (11, (raw, src, dict()), capi.ERR_BAD_ARGUMENT, "keeps raw points"),
        )
        for rule, (d, s, kw), status, text in cases:
            rc, err = call(d, s, **kw)
            assert rc == status and text in err, (rule, rc, err)
            assert checkpoint_bytes(dst) == dst_bytes and checkpoint_bytes(raw) == raw_bytes, rule
        assert call(None, src)[0] == call(dst, None)[0] == capi.ERR_BAD_ARGUMENT          # rule 1
        assert lib.vgicp_map_merge(dst._h, src._h, None, None) == capi.ERR_BAD_ARGUMENT and "NULL pointer" in dst.last_error()
        assert checkpoint_bytes(dst) == dst_bytes and checkpoint_bytes(src) == src_bytes
        # a source that keeps raw points is only read; a radius of 0 is not refused
        assert call(dst, raw, radius=0.0)[0] == capi.OK
    finally:
        empty.close()
        raw.close()


# ---- 9. determinism -------------------------------------------------------------------------------------------------------------
def collision_free_pair(dst, src):
    """dst's keys, and src's keys moved by a whole-voxel shift, all with home slots of their own in dst's table; src's
    keys with home slots of their own in src's: every key sits at its home whatever the order of the claims."""
    slots = next_pow2(4 * 4000)
    shift = np.array([2, -1, 3], dtype=np.int32)
    keys, _ = collision_free(cube(-13, 13, seed=81), slots)
    a, b = keys[0:3000:2], keys[1:2400:2]
    b = np.concatenate([b, a[:400]])                                    # 400 destinations exist already
    moved_from, _ = collision_free(b - shift, slots)
    upsert_map(dst, a, seed=82, hint=4000)
    # counted_map's recipe (1 .. 5 points per key through vgicp_map_insert_scan), into a table of dst's size
    rng = np.random.default_rng(83)
    k = np.repeat(moved_from.astype(np.int64), rng.integers(1, 6, size=len(moved_from)), axis=0)
    pts = ((k + rng.uniform(0.1, 0.9, size=k.shape)) * VOXEL)[rng.permutation(len(k))]
    src.map_reset(VOXEL, 4000)
    src.map_insert_scan(pts, synth.disc_covariances(84, 16, np.arange(len(pts), dtype=np.uint64)), np.eye(4), 6)
    assert dst.map_size() == (len(a), slots) and src.map_size() == (len(moved_from), slots)
    frame = np.eye(4)
    frame[:3, 3] = shift * VOXEL
    return frame


def test_two_identically_built_pairs_give_the_same_checkpoint(three):
    dst, src, dst2 = three
    src2 = capi.Context(0)
    try:
        frame = collision_free_pair(dst, src)
        assert np.array_equal(frame, collision_free_pair(dst2, src2))
        assert checkpoint_bytes(dst) == checkpoint_bytes(dst2) and checkpoint_bytes(src) == checkpoint_bytes(src2)
        st, st2 = dst.map_merge(src, frame=frame, max_count=3), dst2.map_merge(src2, frame=frame, max_count=3)
        assert (st.created, st.updated, st.frozen, st.points) == (st2.created, st2.updated, st2.frozen, st2.points)
        assert st.created > 500 and st.updated > 100
        assert checkpoint_bytes(dst) == checkpoint_bytes(dst2)
    finally:
        src2.close()


# ---- 10. a short walk -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_a_walk_of_insertions_evictions_and_merges(three, seed):
    """Every step is replayed on the exports: an insertion is the fold with every count 1 (tests/test_map_merge_cpu.py pins
    that against the oracle), an eviction is the submap reference's distance test."""
    dst, src, third = three
    rng = np.random.default_rng(100 + seed)
    counted_map(dst, cube(-3, 4, take=250, seed=seed), seed=seed + 10)
    counted_map(src, cube(-4, 5, take=400, seed=seed + 1), seed=seed + 20)
    merges = 0
    for step in range(12):
        op = ("merge", "insert_dst", "evict_dst", "insert_src")[int(rng.integers(0, 4))] if step not in (3, 8) else "merge"
        what = f"seed {seed} step {step} {op}"
        if op in ("insert_dst", "insert_src"):
            ctx = dst if op == "insert_dst" else src
            n, cap = int(rng.integers(50, 400)), int(rng.integers(1, 7))
            pts = rng.uniform(-3.0, 3.0, size=(n, 3))
            covs = synth.disc_covariances(seed + step, 16, np.arange(n, dtype=np.uint64))
            want = mm.merge(ctx.map_export(), pts, covs, np.ones(n, dtype=np.uint64), VOXEL, cap)
            assert ctx.map_insert_scan(pts, covs, np.eye(4), cap) == want.created, what
            assert mm.exports_equal(ctx.map_export(), want.export()), what
        elif op == "evict_dst":
            center, distance = rng.uniform(-1.0, 1.0, size=3), float(rng.uniform(1.5, 3.0))
            k, m, c, n = dst.map_export()
            keep = ~ms.too_far(k, VOXEL, center, distance)
            assert dst.map_evict(center, distance) == int((~keep).sum()), what
            assert mm.exports_equal(dst.map_export(), (k[keep], m[keep], c[keep], n[keep])), what
        else:
            frame = frame_of(float(rng.uniform(-40, 40)), float(rng.uniform(-15, 15)), tuple(rng.uniform(-1.0, 1.0, size=3)))
            center = tuple(rng.uniform(-0.5, 0.5, size=3))
            radius = INF if rng.integers(0, 2) else float(rng.uniform(1.0, 3.0))
            min_count, max_count = int(rng.integers(0, 4)), int((0, 2, 6, 40)[int(rng.integers(0, 4))])
            want, sub = merged_reference(dst, src, third, center, radius, frame, min_count, max_count)
            st = dst.map_merge(src, center, radius, frame, min_count, max_count)
            assert_is_the_rule(dst, st, want, sub, what)
            merges += 1
    assert merges >= 2


# ---- 11. the purpose, end to end ---------------------------------------------------------------------------------------------------
def test_a_second_session_merged_by_the_registered_pose_adds_its_ground(three, oracle):
    """ICP::alignSubmap's recipe finds B's pose in A's map; B is merged into A by it; one of B's sweeps then finds more
    voxels on the merged map than on A alone — exactly as many as numpy counts on the reference-merged map: voxel
    membership of the transformed points decides a correspondence."""
    target, source, third = three
    a_frames, b_frames, D, anchor = ms.two_sessions(oracle)
    for ctx, frames in ((target, a_frames), (source, b_frames)):
        ctx.map_reset(ms.VOXEL, 10000)
        for p, c, pose in frames:
            ctx.map_insert_scan(p, c, pose, ms.CAP)
    sub = target.scan_from_map(source, anchor[:3, 3], ms.RADIUS, synth.invert_pose(anchor), min_count=ms.MIN_COUNT)
    got = target.align_resident(anchor, **ms.ALIGN)
    assert sub.points > 1000 and ms.anchor_error(got.pose, D, anchor) < ms.VOXEL / 2
    b_to_a = got.pose @ synth.invert_pose(anchor)
    p, c, pose_b = b_frames[-1]
    sweep_pose = b_to_a @ pose_b
    # the oracle: this sweep sees ground that A lacks
    omap = oracle.OracleMap(ms.VOXEL, ms.CAP)
    for q, cq, pose in a_frames:
        omap.insert(*oracle.transform(q, cq, pose))
    on_a_oracle = len(omap.match(*oracle.transform(p, c, sweep_pose))[0])
    assert 0 < on_a_oracle < len(p) - 100
    target.scan_upload(p, c)
    on_a = target.evaluate_resident([sweep_pose])[0].correspondences
    assert on_a == on_a_oracle
    want, from_map = merged_reference(target, source, third, frame=b_to_a)
    st = target.map_merge(source, frame=b_to_a)
    assert_is_the_rule(target, st, want, from_map, what="end to end")
    moved, _ = ms.transform(p, c, sweep_pose)
    have = {tuple(k) for k in want.keys.tolist()}
    on_merged_numpy = sum(1 for k in mm.voxel_keys(moved, ms.VOXEL).tolist() if tuple(k) in have)
    on_merged = target.evaluate_resident([sweep_pose])[0].correspondences
    print(f"merge of {st.selected} voxels ({st.points} points): created {st.created} updated {st.updated}; the sweep's correspondences "
          f"{on_a} -> {on_merged} of {len(p)}; {st.launches} launches, {1e6 * st.device_seconds:.1f} us on the device, {1e6 * st.seconds:.1f} us wall")
    assert on_merged == on_merged_numpy > on_a
