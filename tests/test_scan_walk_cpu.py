"""The model of the scan walks (tests/scan_walk_reference.py) on its own, and what makes the committed seeds worth running
on a device.  No GPU needed.

1. The model against the references it is made of: a walk of sources only, the scan the model holds after each against the
   oracle chain written out here (transform, deskew, preprocess; the submap rule on the source's export), its ticket
   numbers, its capacity rule and its checksums against tests/test_gpu_parity.py's.
2. Every committed seed's walk on the model alone: the conditions of `conditions` below, printed with their figures.  They
   are conditions, not measurements: a seed that fails one is replaced, not excused.
3. The committed walks together would see each break of ScanModel.BREAKS."""
import numpy as np
import pytest

import map_submap_reference as msub
import map_walk_reference as mw
import scan_walk_reference as sw
from scan_walk_reference import Op


# ---- 1. the model against the references it is made of --------------------------------------------------------------
def step(d, i, op):
    d.model.begin(i, op)
    d.read(op.kind[5:], op) if op.kind.startswith("read_") else d.apply(op)
    d.model.end()
    return d.model.records[-1]


def test_sources_only_then_download(oracle):
    """One source of every kind in a row, with and without extrinsic and deskew: what scan_download must deliver after
    each is the oracle chain on the scene's sweep, and what scan_info must answer its counts."""
    seed = 7
    d = sw.Driver(oracle, seed, False)
    scene = sw.Scene(oracle, seed)           # a scene of the test's own: nothing cached by the driver
    eye = lambda n: np.tile(np.eye(3).reshape(9), (n, 1))   # noqa: E731
    step(d, 0, Op("reset"))

    def chain(k, ext, deskew, cloud2=False):
        raw = scene._raw(sw.RAW_SIZES[(seed + k) % 8], k)
        if cloud2:
            raw = raw.astype(np.float32).astype(np.float64)
        st = scene.states
        pts, done = raw, 0
        if ext:
            pts, _ = oracle.transform(pts, eye(len(pts)), scene.ext)
        if deskew:
            from eskf_lio_amd import synth
            pts, done = oracle.deskew(pts, synth.make_point_times(len(pts), st[1, 0] + 1e-4, st[-3, 0] + 0.4 / 400.0, seed=k), st)
            assert done > 0
        p, c, _, bad = oracle.preprocess_ex(pts, sw.PREP_VOXEL, sw.KNN)
        return p, c, (len(p), done, bad)

    def holds(p, c, info, source):
        s = d.model.scan
        assert mw.same_bits(s.points, p) and mw.same_bits(s.covs, c) and s.info == info and s.source == source, (source, s.info, info)

    rec = step(d, 1, Op("upload", scan=0))
    p, c, _ = oracle.preprocess(scene._raw(sw.UPLOAD_RAW, 0), sw.UPLOAD_VOXEL, sw.KNN)
    n = sw.UPLOAD_SIZES[(seed + 0) % 8]
    holds(p[:n], c[:n], (n, 0, 0), "upload")
    assert rec.replaced and not rec.realloc and d.model.capacity == ((max(n + n // 4, 1024) + 63) & ~63)
    for i, (kind, k, draw) in enumerate((("prepare", 1, 0.8), ("prepare_async", 2, 0.3), ("prepare", 3, 0.6), ("prepare_async", 4, 0.1))):
        ext, deskew = sw.variant(draw)
        assert (ext, deskew) == ((True, True), (True, False), (False, True), (False, False))[i]
        rec = step(d, 2 + i, Op(kind, scan=k, draw=draw))
        holds(*chain(k, ext, deskew), kind)
        assert rec.replaced and rec.after == ("pending" if kind == "prepare_async" else "settled")
    # a ticket: numbered from 1, prepared with the variant it was staged for, used once
    rec = step(d, 6, Op("stage_cloud2", scan=5, draw=0.6))
    assert not rec.replaced and [t.number for t in d.model.tickets] == [1]
    rec = step(d, 7, Op("prepare_staged"))
    holds(*chain(5, False, True, cloud2=True), "stage_cloud2")
    assert rec.replaced and d.model.tickets == [] and d.model.used == [1] and d.model.busy == 1
    assert step(d, 8, Op("prepare_staged")).error == sw.NO_TICKET_PREPARE and step(d, 9, Op("unstage")).error == sw.NO_TICKET_UNSTAGE
    # a region of the source's map: the submap rule on what an OracleMap of the source's scans exports
    rec = step(d, 10, Op("from_map", scan=6, draw=0.0))
    om = oracle.OracleMap(sw.VOXEL, d.model.src.cap)
    for k in range(sw.SRC_SCANS):
        s = scene.upload(900 + k, 1500)
        om.insert(*oracle.transform(s.points, s.covs, scene.pose(k)))
    pose = scene.at(6)
    from eskf_lio_amd import synth
    want = msub.submap(*mw.sorted_export(om), sw.VOXEL, pose[:3, 3], 5.0, synth.invert_pose(pose), 0)
    holds(want.points, want.covs, (len(want), 0, 0), "from_map")
    assert len(want) > 50 and np.array_equal(d.model.scan.keys, want.keys) and d.model.keys_current and rec.replaced
    assert step(d, 11, Op("from_map", "empty", scan=7)).after == "none" and d.model.keys_current
    for i, kind in enumerate(("align_fused", "accumulate")):
        rec = step(d, 12 + i, Op(kind, scan=8 + i))
        n = sw.UPLOAD_SIZES[(seed + 8 + i) % 8]
        p, c, _ = oracle.preprocess(scene._raw(sw.UPLOAD_RAW, 8 + i), sw.UPLOAD_VOXEL, sw.KNN)
        holds(p[:n], c[:n], (n, 0, 0), kind)
        assert rec.replaced and not d.model.keys_current
    assert d.model.replacements == 10 and all(d.model.seen["generation_" + c] for c in ("upload", "prepare", "from_map"))


def test_the_three_outcomes_that_leave_no_scan(oracle):
    d = sw.Driver(oracle, 7, False)
    step(d, 0, Op("reset"))
    step(d, 1, Op("upload", scan=0))
    rec = step(d, 2, Op("prepare_async", "refused", scan=1))
    assert rec.error is None and rec.after == "refused" and rec.replaced            # only enqueued: nothing is known yet
    rec = step(d, 3, Op("read_download"))
    assert rec.error == sw.REFUSED and rec.surfaced and rec.after == "none"
    assert step(d, 4, Op("read_download")).error == sw.NO_SCAN_DOWNLOAD and d.model.seen["settle_scan"]
    step(d, 5, Op("upload", scan=2))
    rec = step(d, 6, Op("prepare", "unbracketed", scan=3))
    assert rec.error == sw.UNBRACKETED and rec.after == "none" and rec.replaced
    assert step(d, 7, Op("read_info")).error == sw.NO_SCAN_INFO
    for name in ("align", "batch", "evaluate", "points", "rays"):
        assert step(d, 8, Op("read_" + name)).error == sw.NO_SCAN
    assert step(d, 9, Op("insert_resident_async")).error == sw.NO_SCAN
    # a refusal still pending is reported by the source that settles first, which then does nothing else
    step(d, 10, Op("prepare_async", "refused", scan=4))
    rec = step(d, 11, Op("upload", scan=5))
    assert rec.error == sw.REFUSED and not rec.replaced and rec.after == "none"


def test_fetch_rules(oracle):
    """The rules in the comment of vgicp_scan_fetch_begin / _end / _sums, on the model."""
    d = sw.Driver(oracle, 7, False)
    m = d.model
    step(d, 0, Op("reset"))
    step(d, 1, Op("prepare_async", scan=0))
    step(d, 2, Op("read_fetch_begin"))
    assert m.fetch_open and m.pending == "good"                                      # the begin settles nothing
    assert step(d, 3, Op("read_fetch_end")).error is None and m.sums_valid and m.pending is None
    assert step(d, 4, Op("read_fetch_sums")).error is None
    step(d, 5, Op("read_fetch_begin"))                                               # nothing pending: the two-step path
    assert not m.fetch_open and not m.sums_valid
    assert step(d, 6, Op("read_fetch_end")).error is None and step(d, 7, Op("read_fetch_sums")).error == sw.NO_SUMS
    step(d, 8, Op("prepare_async", scan=1))
    step(d, 9, Op("read_fetch_begin"))
    step(d, 10, Op("read_align"))                                                    # reads the scan, leaves it resident
    assert m.fetch_open and step(d, 11, Op("read_fetch_end")).error is None and m.sums_valid
    step(d, 12, Op("upload", scan=2))                                                # a replacement voids the sums
    assert step(d, 13, Op("read_fetch_sums")).error == sw.NO_SUMS and m.seen["forget_fetch"]


def test_checksums_restate_the_header(oracle):
    from test_gpu_parity import _assert_fetch_sums
    s = sw.Scene(oracle, 3).upload(0, 777)
    _assert_fetch_sums(sw.expected_sums(s.points, s.covs), s.points, s.covs, "model")


def test_walk_shape():
    for seed in sw.SEEDS:
        ops = sw.walk(seed, False)
        names = [o.kind + (":" + o.arg if o.arg else "") for o in ops]
        assert len(ops) == sw.WALK_LENGTH and tuple(names[:len(sw.PREFIX)]) == sw.PREFIX
        assert [repr(o) for o in sw.walk(seed, True)] == [repr(o) for o in ops]       # the store changes no operation
        kinds = {o.kind for o in ops}
        for kind in sw.SOURCES + sw.DEFERRED + sw.BYSTANDERS + ("prepare_staged", "unstage") + tuple("read_" + r for r in sw.SETTLING[:2]):
            assert kind in kinds, kind
        # every fragment is there, in one piece, and no full check falls inside one
        settling = {"read_" + r for r in sw.SETTLING}
        for f in sw.FRAGMENTS:
            at = [i for i in range(len(ops)) if all(i + j < len(ops) and (names[i + j] == f[j] or (f[j] == "R" and names[i + j] in settling))
                                                    for j in range(len(f)))]
            assert at and any(i // sw.FULL_CHECK_EVERY == (i + len(f) - 1) // sw.FULL_CHECK_EVERY for i in at), f
        sizes = [o.scan for o in ops if o.scan >= 0]
        assert sizes == list(range(len(sizes)))


# ---- 2. the committed seeds -----------------------------------------------------------------------------------------
def conditions(model):
    """-> (the list of conditions the walk fails, the figures they were checked on)."""
    rs = model.records
    failed, fig = [], {}
    reader = lambda r: r.kind.startswith(("read_", "full_"))                         # noqa: E731
    name = lambda r: r.kind.split("_", 1)[1] if reader(r) else r.kind               # noqa: E731
    pairs = list(zip(rs, rs[1:]))
    triples = list(zip(rs, rs[1:], rs[2:]))

    # the stale tail
    fig["smaller_then_reader"] = [(a.i, a.n_before, a.n_after) for a, b in pairs
                                  if a.replaced and 0 < a.n_after < a.n_before and reader(b) and b.error is None and name(b) != "generation"]
    fig["larger"] = sum(1 for a in rs if a.replaced and a.n_after > a.n_before > 0)
    fig["realloc_under_insertion"] = [(a.i, a.kind) for a in rs if a.realloc and a.deferred_before == "insert_resident_async"]
    for what in ("smaller_then_reader", "larger", "realloc_under_insertion"):
        if not fig[what]:
            failed.append(what)
    # a fetch across a replacement
    across = {}
    for a, b, c in triples:
        if a.replaced and a.fetch_open_before and a.before == "pending" and a.arg != "refused" and a.error is None \
                and name(b) == "fetch_end" and b.error is None and name(c) == "fetch_sums" and c.error == sw.NO_SUMS:
            across.setdefault(a.kind, []).append((a.i, a.fetched_n, a.n_after))
    fig["fetch_across"] = across
    for kind in ("upload", "prepare_async", "align_fused"):
        if kind not in across:
            failed.append("no fetch across " + kind)
    if not any(kept == n for v in across.values() for _, kept, n in v):
        failed.append("no replacing scan has exactly as many points as the fetched one kept")
    # deferred totals in a preparation's copy
    travelled = {}
    for a, b, c in triples:
        if a.kind in ("prepare_async", "prepare_staged") and a.replaced and a.error is None and a.deferred_before \
                and name(b) in ("info", "align") and b.totals_via == "prep" and b.error is None and name(c) == "map":
            travelled.setdefault(a.deferred_before, []).append((a.i, a.kind, name(b)))
    fig["totals_with_a_preparation"] = travelled
    for kind in sw.DEFERRED:
        if kind not in travelled:
            failed.append(f"the totals of no {kind} travel with a preparation")
    if {k for v in travelled.values() for _, k, _ in v} != {"prepare_async", "prepare_staged"}:
        failed.append("not both of prepare_async and prepare_staged carry totals")
    changed = {}
    for r in rs:
        if r.map_event is not None:
            e = r.map_event
            changed[r.kind] = changed.get(r.kind, 0) + len(e.created) + e.removed + e.refused
    fig["deferred_changes"] = changed
    for kind in sw.DEFERRED:
        if not changed.get(kind):
            failed.append(f"{kind} changes nothing")
    gaps = [r.map_event.gap / (mw.GAP_FACTOR * r.map_event.gap_bound) for r in rs if r.kind == "gated_async" and r.map_event is not None]
    fig["smallest_gap_in_bounds"] = min(gaps) * mw.GAP_FACTOR if gaps else None
    if not gaps or not min(gaps) > 1.0:
        failed.append("a gated step has no gap of 1000 bounds")
    # two preparations in a row, nothing settled between
    fig["replaces_a_pending_scan"] = [a.i for a in rs if a.kind in ("prepare_async", "prepare_staged") and a.replaced and a.before == "pending"]
    if not fig["replaces_a_pending_scan"]:
        failed.append("no preparation replaces a pending scan")
    # a refused preparation
    recovered = {}
    for a, b, c in triples:
        if a.kind == "prepare_async" and a.arg == "refused" and reader(b) and b.surfaced and b.after == "none" \
                and c.replaced and c.error is None and c.before == "none" and c.after in ("settled", "pending"):
            recovered.setdefault(c.source, []).append(a.i)
    fig["recovered_by"] = recovered
    for kind in sw.SOURCES:
        if kind not in recovered:
            failed.append("no recovery from a refusal by " + kind)
    fig["refused_with_a_fetch_open"] = [a.i for a in rs if a.arg == "refused" and a.fetch_open_before]
    if not fig["refused_with_a_fetch_open"]:
        failed.append("no refused preparation with a fetch open")
    fig["no_scan_outcomes"] = sorted({(a.kind, a.arg or a.note) for a in rs if a.replaced and a.after == "none" and not a.surfaced} |
                                     {(a.kind, a.arg) for a in rs if a.after == "refused" and a.replaced})
    if fig["no_scan_outcomes"] != [("from_map", "empty"), ("prepare", "unbracketed"), ("prepare_async", "refused")]:
        failed.append("not the three outcomes that leave no scan")
    # tickets
    errors = lambda kind, arg, err: [a.i for a in rs if a.kind == kind and a.arg == arg and a.error == err]   # noqa: E731
    fig["tickets"] = dict(fourth=errors("stage", "", sw.SLOTS_FULL), dropped=errors("prepare_staged", "dropped", sw.NO_TICKET_PREPARE),
                          used=errors("unstage", "used", sw.NO_TICKET_UNSTAGE),
                          survives=[a.i for a, b in pairs if a.error == sw.NO_TIMES and b.kind == "prepare_staged" and b.error is None and b.replaced],
                          across=[a.i for a in rs if a.kind == "prepare_staged" and a.replaced and a.ticket_age >= 1])
    for what, where in fig["tickets"].items():
        if not where:
            failed.append("tickets: " + what)
    if not any(a.error == sw.SLOTS_FULL and a.note == "3 staged" for a in rs):
        failed.append("the refused staging is not the fourth of three staged")
    # from_map onto a pending preparation, the source with an insertion pending
    fig["from_map_onto_pending"] = [a.i for a in rs if a.kind == "from_map" and a.arg == "pending" and a.before == "pending" and a.error is None]
    if not fig["from_map_onto_pending"]:
        failed.append("no from_map onto a pending preparation")
    # both align paths read a scan from every kind of source (the align reader takes both)
    aligned = {}
    for r in rs:
        if name(r) == "align" and reader(r) and r.error is None:
            aligned.setdefault(r.source, []).append(int(r.note))
    fig["aligned"] = {k: (len(v), min(v)) for k, v in aligned.items()}
    for kind in sw.SOURCES:
        if kind not in aligned:
            failed.append("no align of a scan from " + kind)
    if aligned and min(min(v) for v in aligned.values()) < 10:
        failed.append("an align has fewer than 10 correspondences")
    # a bystander between a deskewed preparation and scan_info
    fig["preprocess_then_info"] = [b.i for a, b, c in triples if a.kind in ("prepare_async", "prepare") and b.kind == "preprocess" and b.error is None
                                   and name(c) == "info" and c.error is None and a.note == "deskewed"]
    if not fig["preprocess_then_info"]:
        failed.append("no preprocess between a deskewed preparation and scan_info")
    return failed, fig


@pytest.fixture(scope="module")
def walked(oracle):
    return {seed: sw.run_walk(oracle, seed, False) for seed in sw.SEEDS}


@pytest.mark.parametrize("seed", sw.SEEDS)
def test_committed_seed_is_worth_running(oracle, walked, seed):
    model = walked[seed]
    failed, figures = conditions(model)
    print(f"seed {seed} cap {model.map.cap}: {model.implied} comparisons implied, map voxels {model.map.voxels}; breaks a reader of this "
          f"walk would see: {sorted(k for k, v in model.seen.items() if v)}")
    for name, value in figures.items():
        print(f"  {name}: {value}")
    assert not failed, failed
    # the raw walk is the same walk: the store changes no decision, and adds the reader of the per-voxel lists
    raw = sw.run_walk(oracle, seed, True)
    assert [(r.kind, r.error, r.after, r.n_after) for r in raw.records] == [(r.kind, r.error, r.after, r.n_after) for r in model.records]
    assert raw.implied == model.implied + sum(1 for r in model.records if r.kind in ("read_map", "full_map"))


def test_the_committed_walks_together_would_see_each_break(walked):
    """ScanModel.BREAKS: the model keeps for each what a library broken that way would hold and notes where a reader of the
    walk would get another answer.  Every break must be visible in at least one committed walk."""
    seen = {}
    for seed, model in walked.items():
        for what, would in model.seen.items():
            seen.setdefault(what, []).extend([seed] if would else [])
    print(f"seeds whose walk would see each break: {seen}")
    assert set(seen) == set(sw.ScanModel.BREAKS) and all(seen.values()), seen
