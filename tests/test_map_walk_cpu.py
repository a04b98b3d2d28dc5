"""The model of the map walks (tests/map_walk_reference.py) on its own, and what makes the committed seeds worth running
on a device.  No GPU needed.

1. The model against the references it is made of: a walk of insertions only is one OracleMap fed the same scans (and
   test_map_raw_points.py's RawMap, for the raw lists); a removal followed by a re-insertion is an OracleMap that never saw
   the removed points; the `slots` rule on the cases tests/native/map_plan.cpp enumerates for the table's growth.
2. Every committed seed's walk on the model alone: the conditions of `conditions` below.  They are conditions, not
   measurements: a seed that fails one is replaced, not excused."""
import numpy as np
import pytest

import map_walk_reference as mw
from test_map_raw_points import RawMap


def oracle_export(om):
    return mw.sorted_export(om)


def assert_same_export(got, want):
    for what, g, w in zip(("keys", "means", "covs", "counts"), got, want):
        assert mw.same_bits(g, w), what


# ---- 1. the model against the references it is made of --------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3, 20])
def test_insertions_only_equal_one_oracle_map(oracle, cap):
    scene = mw.Scene(oracle, 5)
    model = mw.Model(oracle, cap)
    om, rm = oracle.OracleMap(mw.VOXEL, cap), RawMap(oracle, mw.VOXEL)
    news = []
    for k in range(4):
        s = scene.scan(k, prepared=k % 2 == 1)
        before = len(om)
        wp, wc = oracle.transform(s.points, s.covs, s.pose)
        om.insert(wp, wc)
        rm.insert(wp, cap)
        ev, new = model.insert("insert_scan", s.points, s.covs, s.pose)
        news.append(new)
        assert new == len(om) - before and model.voxels == len(om)
    assert_same_export(model.export(), oracle_export(om))
    lists = model.raw_lists()
    assert set(lists) == set(rm.vox)
    for k, want in rm.vox.items():
        assert mw.same_bits(lists[k], np.asarray(want)), k
    if cap > 1:
        assert max(len(v) for v in lists.values()) > 1
    assert news[0] > 0 and min(news) >= 0


def test_a_removed_key_starts_afresh(oracle):
    """Insert A, remove a tenth of the keys (erase) and what an eviction takes, insert A again and B: the map an
    OracleMap has that was never shown A's points of the removed keys."""
    cap = 4
    scene = mw.Scene(oracle, 6)
    a, b = scene.scan(0, False), scene.scan(1, True)
    model = mw.Model(oracle, cap)
    model.insert("insert_scan", a.points, a.covs, a.pose)
    victims = mw.erased_tenth(model.keys, 0.37)
    ev = model.erase(victims)
    assert ev.removed == len(victims) > 0 and model.tombstones == len(victims)
    ev2 = model.evict(a.pose[:3, 3], 7.0)
    assert ev2.removed > 0 and model.tombstones == len(victims) + ev2.removed
    gone = ev.removed_codes | ev2.removed_codes
    ev3, new = model.insert("insert_scan", a.points, a.covs, a.pose)
    assert ev3.created == gone and new == len(gone)          # the same scan again: exactly the removed keys return
    model.insert("insert_resident", b.points, b.covs, b.pose)
    # the reference: A without the points of the removed keys, then A, then B
    wp, wc = oracle.transform(a.points, a.covs, a.pose)
    stays = ~np.isin(mw.code_of(oracle.voxel_index(mw.VOXEL, wp)), np.array(sorted(gone)))
    om = oracle.OracleMap(mw.VOXEL, cap)
    om.insert(wp[stays], wc[stays])
    om.insert(wp, wc)
    om.insert(*oracle.transform(b.points, b.covs, b.pose))
    assert_same_export(model.export(), oracle_export(om))
    # ... and the eviction took what OracleMap.evict takes
    om2 = oracle.OracleMap(mw.VOXEL, cap)
    om2.insert(wp, wc)
    centres = (om2.export()[0].astype(np.float64) + 0.5) * mw.VOXEL
    far = np.sqrt(((centres - a.pose[:3, 3]) ** 2).sum(axis=1)) > 7.0
    assert ev2.removed_codes == set(mw.code_of(om2.export()[0][far]).tolist()) - ev.removed_codes


# (slots, voxels, incoming, tombstones) -> (grows, slots after): tests/native/map_plan.cpp's enumeration of the table's
# growth with nothing pending — the load at slots / 2 and one past, carried by voxels, incoming and tombstones in turn —
# worked out by hand from plan_table_growth / table_for
GROWTH_CASES = [
    ((1024, 512, 0, 0), (False, 1024)), ((1024, 513, 0, 0), (True, 4096)),
    ((1024, 0, 512, 0), (False, 1024)), ((1024, 0, 513, 0), (True, 4096)),
    ((1024, 0, 0, 512), (False, 1024)), ((1024, 0, 0, 513), (True, 1024)),            # the tombstones stay behind
    ((1 << 20, 1 << 19, 0, 0), (False, 1 << 20)), ((1 << 20, (1 << 19) + 1, 0, 0), (True, 1 << 22)),
    ((1 << 20, 0, 1 << 19, 0), (False, 1 << 20)), ((1 << 20, 0, (1 << 19) + 1, 0), (True, 1 << 22)),
    ((1 << 20, 0, 0, 1 << 19), (False, 1 << 20)), ((1 << 20, 0, 0, (1 << 19) + 1), (True, 1024)),
    ((8192, 2000, 1500, 597), (True, 16384)), ((8192, 2000, 1500, 596), (False, 8192)),   # all three at once
    ((8192, 2597, 1500, 0), (True, 32768)),
]


@pytest.mark.parametrize("case, want", GROWTH_CASES)
def test_slots_rule(case, want):
    slots, voxels, incoming, tombstones = case
    grew, after, left = mw.table_growth(slots, voxels, tombstones, incoming)
    assert (grew, after) == want
    assert left == (0 if grew else tombstones)


def test_reset_and_walk_shape():
    assert mw.next_pow2(max(mw.MIN_SLOTS, 0)) == 1024
    for seed in mw.SEEDS:
        for raw in (False, True):
            ops = mw.walk(seed, raw)
            kinds = [o.kind for o in ops]
            assert len(ops) == mw.WALK_LENGTH == 48 and kinds[:3] == ["reset", "upload", "insert_resident"]
            for kind, count in mw.MULTISET:
                assert kinds[3:].count(kind) == count, kind
            assert sum(k.startswith("read_") for k in kinds) == 10
            assert ("read_points" in kinds) <= raw
        assert [o.kind.replace("read_points", "read_export") for o in mw.walk(seed, True)] == [o.kind for o in mw.walk(seed, False)]


# ---- 2. the committed seeds -----------------------------------------------------------------------------------------
def conditions(seed, ops, events, level_sizes):
    """-> (the list of conditions the walk fails, the figures they were checked on)."""
    kinds = [o.kind for o in ops]
    failed = []
    total = {}
    for _, e in events:
        t = total.setdefault(e.kind, dict(removed=0, refused=0, kept=0))
        t["removed"] += e.removed
        t["refused"] += e.refused
        t["kept"] += e.kept
    for kind in ("carve", "carve_async", "evict", "erase"):
        if not total[kind]["removed"] > 0:
            failed.append(f"{kind} removes nothing")
    for kind in ("gated", "gated_async"):
        if not (total[kind]["refused"] > 0 and total[kind]["kept"] > 0):
            failed.append(f"{kind} refuses or keeps nothing")
    gone, returned = set(), 0
    for _, e in events:
        returned += len(e.created & gone)
        gone |= e.removed_codes
    if returned == 0:
        failed.append("no removed key is created again")
    grows = [(i, e) for i, e in events if e.grew]
    if len(grows) < 2:
        failed.append("the table grows fewer than two times")
    if not any(e.tombstones_before > 0 for _, e in grows):
        failed.append("the table never grows with tombstones in it")
    if not any(a in mw.DEFERRED and b in mw.DEFERRED and a != b for a, b in zip(kinds, kinds[1:])):
        failed.append("no deferred operation is directly followed by a deferred operation of another kind")
    if not any(kinds[i - 1] == "carve_async" and e.kind in mw.INSERTIONS for i, e in grows):
        failed.append("no deferred carve is directly followed by an insertion that grows the table")
    ratios = [e.gap / (mw.GAP_FACTOR * e.gap_bound) for _, e in events if e.kind in ("gated", "gated_async")]
    if len(ratios) != 6 or not min(ratios) > 1.0:
        failed.append("a gated step has no gap of 1000 bounds")
    built = max(int(o.draw * 4) for o in ops if o.kind == "levels")
    if built < 1:
        failed.append("no level is built")
    for l in range(1, built + 1):
        if not any(sizes[l] < sizes[l - 1] for sizes in level_sizes):
            failed.append(f"level {l} never holds fewer voxels than level {l - 1}")
    figures = dict(totals=total, grows=[(i, e.kind, e.tombstones_before) for i, e in grows], returned_keys=returned,
                   smallest_gap_in_bounds=min(ratios) * mw.GAP_FACTOR if ratios else None, levels_built=built,
                   level_sizes_at_end=level_sizes[-1])
    return failed, figures


@pytest.mark.parametrize("seed", mw.SEEDS)
def test_committed_seed_is_worth_running(oracle, seed):
    ops = mw.walk(seed, False)
    model, events, level_sizes = mw.run_walk(oracle, seed, False, ops=ops)
    failed, figures = conditions(seed, ops, events, level_sizes)
    print(f"seed {seed} cap {model.cap}: voxels {model.voxels} slots {model.slots} tombstones {model.tombstones}; "
          f"breaks a reader of this walk would see: {sorted(k for k, v in model.seen.items() if v)}")
    for name, value in figures.items():
        print(f"  {name}: {value}")
    assert not failed, failed
    assert len(level_sizes) == mw.WALK_LENGTH // mw.FULL_CHECK_EVERY
    # the raw walk is the same walk: the store changes no decision
    model_raw, events_raw, _ = mw.run_walk(oracle, seed, True)
    assert [(i, e.kind, e.grew, e.removed, e.refused) for i, e in events_raw] == [(i, e.kind, e.grew, e.removed, e.refused) for i, e in events]


def test_the_committed_walks_together_would_see_each_break(oracle):
    """Three ways to break the bookkeeping the walks are for (Model.begin names them): the deferred carve does not
    advance map_version, finish_removal leaves the tombstones alone, ensure_table does not settle a pending carve before
    the table grows.  The model keeps the host's counts as each broken library would and notes where a reader of the
    walk would see another answer: a level that is still the map's of before the carve at a `levels` reader, another
    table size at a `size` reader.  Every break must be visible in at least one committed walk."""
    seen = {}
    for seed in mw.SEEDS:
        model, _, _ = mw.run_walk(oracle, seed, False)
        for what, would in model.seen.items():
            seen.setdefault(what, []).extend([seed] if would else [])
    print(f"seeds whose walk would see each break: {seen}")
    assert set(seen) == {"version", "tombstones", "settle"} and all(seen.values()), seen
