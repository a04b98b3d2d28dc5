"""The reference of the map walks: ONE host model of the voxel map behind every update and every reader of the C ABI, the
scene the walks run in, the walks themselves and the driver that holds a device context against the model step by step.
Not a test module; tests/test_map_walk_cpu.py checks the model against the references it is made of and the committed
seeds' preconditions, tests/test_map_walk.py drives the device.

THE MODEL.  State: the voxel size, the cap (max_points_per_voxel, one per walk), the resident scan as the device holds it,
and a chronological log of the live world points (point, covariance, key, in order of arrival).  World points are the bits
of the oracle's transform.  Everything expected follows from the log: the map is a fresh OracleMap fed the log in order (a
voxel depends on its own points only, so this is exact), the raw store is per key the first `cap` logged points, a removal
deletes the log's entries of the removed keys (a key that returns starts afresh).  `slots` and `tombstones` follow
plan_table_growth / table_for of eskf_lio_amd/csrc/vgicp_map_plan.h.  Every decision (evict, carve, gate) is taken from the
model alone, never from what a device returned.
"""
from dataclasses import dataclass, field

import numpy as np

import map_carve_reference as mc
import map_gated_reference as mg
import map_levels_reference as ml
import map_locate_reference as mloc
import map_rays_reference as mr
import points_reference as pr
from eskf_lio_amd import synth

VOXEL = 0.5
PREP_VOXEL = 0.25             # (ceil(0.5 / 0.25) + 1)^3 = 27 <= 64: a prepared scan's insertion takes the lists route
KNN = 30
UPLOAD_POINTS = 1500
UPLOAD_RAW, UPLOAD_VOXEL = 3200, 0.2      # an uploaded scan: the first UPLOAD_POINTS kept points of such a preparation
PREPARE_RAW = 4000
EXTENT = 12.0
SENSOR_HEIGHT = 1.6
WALK_LENGTH = 48
FULL_CHECK_EVERY = 8
CAPS = (3, 5, 8, 20)          # max_points_per_voxel of a walk: CAPS[seed % 4]
MIN_SLOTS = 1024              # kMinSlots
ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS = 3, 1e-12, 2.0     # three rounds, none converges
ALIGN_OFFSET = (0.04, -0.03, 0.02, 0.003, -0.002, 0.004)
GAP_FACTOR = 1000.0
LOCATE_WINDOW = (1, 1, 1)
RAY_PARAMS = mr.Params(margin=0.25, beyond=1.0, max_range=60.0, stride=1)
EVICT_DISTANCES = (9.0, 7.0)
# The committed seeds: each meets the conditions of tests/test_map_walk_cpu.py; found by running them over the seeds
# 1 .. 999 (about one in twenty meets them all).  One cap each; 896 would see the break "version", 229 "tombstones" and
# "settle" (Model.begin), 34 and 419 "tombstones"
SEEDS = (896, 229, 34, 419)

PREFIX = (("reset",), ("upload",), ("insert_resident",))
MULTISET = (("upload", 3), ("prepare", 3), ("insert_scan", 3), ("insert_resident", 3), ("insert_resident_async", 4),
            ("gated", 3), ("gated_async", 3), ("carve", 3), ("carve_async", 3), ("evict", 2), ("erase", 2), ("levels", 3))
READERS = ("export", "size", "points", "levels", "align", "locate", "rays", "totals")
DEFERRED = ("insert_resident_async", "gated_async", "carve_async")
INSERTIONS = ("insert_scan", "insert_resident", "insert_resident_async", "gated", "gated_async")


# ---- the walk --------------------------------------------------------------------------------------------------------
@dataclass
class Op:
    kind: str
    scan: int = -1            # upload / prepare / insert_scan: the scan's number within the walk
    draw: float = 0.0         # the op's own uniform draw in [0, 1): levels' k, the erased tenth, the carve's parameters

    def __repr__(self):
        return self.kind + (f"#{self.scan}" if self.scan >= 0 else "")


def walk(seed, raw):
    """The 48 operations of a walk: the prefix, then a seeded shuffle of the multiset with a reader in every remaining
    place, so every kind occurs in every walk.  raw: the walk's context keeps raw points (the `points` reader reads them;
    without the store it reads the export)."""
    kinds = [k for k, count in MULTISET for _ in range(count)]
    fill = WALK_LENGTH - len(PREFIX) - len(kinds)
    idx = np.arange(WALK_LENGTH, dtype=np.uint64)
    pick = (synth.rand_unit(seed, 901, idx[:fill]) * len(READERS)).astype(np.int64)
    kinds += ["read_" + READERS[p] for p in pick]
    order = np.argsort(synth.rand_u64(seed, 902, idx[:len(kinds)]), kind="stable")
    kinds = [p[0] for p in PREFIX] + [kinds[i] for i in order]
    draws = synth.rand_unit(seed, 903, idx)
    ops, scans = [], 0
    for i, kind in enumerate(kinds):
        if kind == "read_points" and not raw:
            kind = "read_export"
        op = Op(kind, draw=float(draws[i]))
        if kind in ("upload", "prepare", "insert_scan"):
            op.scan, scans = scans, scans + 1
        ops.append(op)
    assert len(ops) == WALK_LENGTH
    return ops


# ---- the scene -------------------------------------------------------------------------------------------------------
@dataclass
class Scan:
    points: np.ndarray        # as the device holds them (a prepared scan: oracle.preprocess's output)
    covs: np.ndarray
    pose: np.ndarray
    raw: np.ndarray = None    # a prepared scan's raw points


class Scene:
    """A ground plane, two walls and clutter around a sensor SENSOR_HEIGHT above the ground (synth.make_lidar_scan, every
    scan its own sample), and a sensor pose that drifts a few decimetres per new scan."""

    def __init__(self, oracle, seed):
        self.oracle, self.seed, self.cache = oracle, seed, {}

    def pose(self, k):
        idx = np.arange(k + 1, dtype=np.uint64)
        u = [synth.rand_unit(self.seed, 910 + a, idx) for a in range(3)]
        xi = [float(np.sum(0.15 + 0.25 * u[0])), float(np.sum(0.4 * u[1] - 0.2)), 0.0, 0.0, 0.0, float(np.sum(0.06 * u[2] - 0.03))]
        return synth.se3_to_SE3(xi)

    def scan(self, k, prepared):
        if (k, prepared) not in self.cache:
            n, voxel = (PREPARE_RAW, PREP_VOXEL) if prepared else (UPLOAD_RAW, UPLOAD_VOXEL)
            raw = synth.make_lidar_scan(n, seed=self.seed * 1000 + k, extent=EXTENT) - np.array([0.0, 0.0, SENSOR_HEIGHT])
            raw = np.ascontiguousarray(raw)
            p, c, _ = self.oracle.preprocess(raw, voxel, KNN)
            if not prepared:
                assert len(p) >= UPLOAD_POINTS, len(p)
                p, c = np.ascontiguousarray(p[:UPLOAD_POINTS]), np.ascontiguousarray(c[:UPLOAD_POINTS])
            self.cache[k, prepared] = Scan(p, c, self.pose(k), raw if prepared else None)
        return self.cache[k, prepared]


# ---- the model -------------------------------------------------------------------------------------------------------
def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def table_growth(slots, voxels, tombstones, incoming):
    """plan_table_growth with a table and nothing pending -> (grows, slots after, tombstones after)."""
    if (voxels + tombstones + incoming) * 2 <= slots:
        return False, slots, tombstones
    return True, next_pow2(max(MIN_SLOTS, 4 * (voxels + incoming))), 0


def code_of(keys):
    """One int64 per key (components within +-2^20: every scene here), ascending in (x, y, z)."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    assert k.size == 0 or np.abs(k).max() < (1 << 20)
    return ((k[:, 0] + (1 << 20)) << 42) | ((k[:, 1] + (1 << 20)) << 21) | (k[:, 2] + (1 << 20))


def sorted_export(om):
    k, m, c, n = om.export()
    order = np.lexsort(k.T)                   # Context.map_export's order
    return k[order], m[order], c[order], n[order]


def gate_of(ref):
    """The gate of a gated step: the midpoint of the widest relative gap of the ranked d^2 between its 0.6 and 0.9
    quantiles -> (gate, that gap, the bound on a d^2's relative error: tests/test_points.py's term_bound)."""
    ranked = ref.ranked
    m = len(ranked)
    assert m >= 10, m
    seg = ranked[pr.quantile_rank(0.6, m):pr.quantile_rank(0.9, m) + 1]
    if not seg[0] > 0.0:
        return float(seg[0]), 0.0, 1.0                # (no gap to speak of: the seed fails its condition)
    rel = (seg[1:] - seg[:-1]) / seg[1:]
    j = int(np.argmax(rel))
    return float(0.5 * (seg[j] + seg[j + 1])), float(rel[j]), pr.COST_C * ref.kappa * ref.kappa * pr.U


@dataclass
class Event:
    """What one operation did to the model (tests/test_map_walk_cpu.py's conditions are stated on these)."""
    kind: str
    grew: bool = False
    tombstones_before: int = 0
    removed: int = 0
    refused: int = 0
    kept: int = 0
    gap: float = float("inf")
    gap_bound: float = 0.0
    created: set = field(default_factory=set)
    removed_codes: set = field(default_factory=set)


class Model:
    def __init__(self, oracle, cap):
        self.oracle, self.cap = oracle, int(cap)
        self.scan = None
        self.levels = 0
        self.seen = dict(version=False, tombstones=False, settle=False)    # see `begin` and `note_reader`
        self.reset(VOXEL, 0)

    # -- state --
    def reset(self, voxel, hint):
        self.voxel = float(voxel)
        self.slots = next_pow2(max(MIN_SLOTS, 4 * int(hint)))
        self.tombstones = 0
        self.log_p, self.log_c = np.zeros((0, 3)), np.zeros((0, 9))
        self.log_k, self.log_code = np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int64)
        self.gated_points = self.gated_refused = self.carve_rays = self.carve_removed = 0
        self._om = self._export = None
        # the host's bookkeeping as three broken libraries would keep it (BREAKS below): (slots, tombstones) of each
        self.broken = {"tombstones": [self.slots, 0], "settle": [self.slots, 0]}
        self.pending_carve, self.last_kind = 0, "reset"
        self.levels_current = self.levels_stale = False

    def _changed(self):
        self._om = self._export = None

    @property
    def om(self):
        if self._om is None:
            self._om = self.oracle.OracleMap(self.voxel, self.cap)
            if len(self.log_p):
                self._om.insert(self.log_p, self.log_c)
        return self._om

    def export(self):
        """(keys, means, covs, counts) sorted by key as Context.map_export sorts."""
        if self._export is None:
            self._export = sorted_export(self.om)
        return self._export

    @property
    def keys(self):
        return self.export()[0]

    @property
    def voxels(self):
        return len(np.unique(self.log_code))

    def raw_lists(self):
        """key (tuple) -> the first `cap` logged points of the voxel, in order of arrival."""
        order = np.argsort(self.log_code, kind="stable")
        code = self.log_code[order]
        starts = np.flatnonzero(np.r_[True, code[1:] != code[:-1]]) if len(code) else np.zeros(0, dtype=np.int64)
        ends = np.r_[starts[1:], len(code)]
        return {tuple(self.log_k[order[s]].tolist()): self.log_p[order[s:min(e, s + self.cap)]] for s, e in zip(starts, ends)}

    def level_list(self, levels=None):
        return ml.levels_of(*self.export(), self.levels if levels is None else levels)

    # -- updates --
    def set_scan(self, scan):
        self.scan = scan

    def _append(self, points, covs, pose, ev):
        wp, wc = self.oracle.transform(points, covs, pose)
        keys = self.oracle.voxel_index(self.voxel, wp)
        code = code_of(keys)
        ev.created = set(np.unique(code).tolist()) - set(np.unique(self.log_code).tolist())
        self.log_p, self.log_c = np.concatenate([self.log_p, wp]), np.concatenate([self.log_c, wc])
        self.log_k, self.log_code = np.concatenate([self.log_k, keys]), np.concatenate([self.log_code, code])
        self._changed()
        return len(ev.created)

    def _room(self, incoming, ev):
        ev.tombstones_before = self.tombstones
        voxels = self.voxels
        ev.grew, self.slots, self.tombstones = table_growth(self.slots, voxels, self.tombstones, incoming)
        for name, st in self.broken.items():
            if name == "settle" and self.pending_carve:
                # the pending carve's share is still counted as voxels when the new table is sized, and becomes
                # tombstones of a table that holds none when it is settled afterwards
                if (voxels + st[1] + incoming) * 2 > st[0]:
                    st[0], st[1] = next_pow2(max(MIN_SLOTS, 4 * (voxels + self.pending_carve + incoming))), self.pending_carve
            else:
                _, st[0], st[1] = table_growth(st[0], voxels, st[1], incoming)

    # -- what a broken library would show (tests/test_map_walk_cpu.py asks that every committed walk would see each) --
    # BREAKS: "version": the deferred carve does not advance map_version; "tombstones": finish_removal (erase, evict)
    # leaves ctx->tombstones alone; "settle": ensure_table does not settle a pending carve before the table grows.
    def begin(self, kind):
        """Every operation of a walk begins here: what is pending on the host when the entry runs, and whether the
        levels are still the map's."""
        deferred_insert = kind in ("insert_resident_async", "gated_async")
        if not (kind == "carve_async" or (deferred_insert and self.last_kind == "carve_async")):
            self.pending_carve = 0            # every other entry settles first
        if kind in INSERTIONS or kind in ("carve", "evict", "erase"):
            self.levels_current = self.levels_stale = False
        self.last_kind = kind

    def note_reader(self, name):
        """A reader ran (they all settle): what it would have seen of each break."""
        self.pending_carve, self.last_kind = 0, "read"
        if name == "size":
            for what, st in self.broken.items():
                self.seen[what] |= st[0] != self.slots
        if name in ("levels", "locate", "build") and self.levels >= 1:
            if name == "levels" and self.levels_current and self.levels_stale:
                self.seen["version"] = True
            if not self.levels_current:
                self.levels_current, self.levels_stale = True, False

    def insert(self, kind, points, covs, pose):
        """An insertion of a whole scan -> (event, new voxels)."""
        ev = Event(kind)
        self._room(len(points), ev)
        return ev, self._append(points, covs, pose, ev)

    def gated(self, kind, pose):
        """A gated insertion of the resident scan at its gate -> (event, gate, kept, (matched, refused, not finite), new voxels)."""
        ev = Event(kind)
        s = self.scan
        ref = pr.reference_at(self.oracle, self.om, s.points, s.covs, pose)
        gate, ev.gap, ev.gap_bound = gate_of(ref)
        d2, _, _, status = ref.planes()
        kept = mg.rule(d2, status, gate)
        counts = mg.counts(status, kept)
        self._room(len(s.points), ev)             # the table makes room for the whole scan
        take = kept != 0
        new = self._append(s.points[take], s.covs[take], pose, ev)
        ev.refused, ev.kept = counts[1], int(take.sum())
        self.gated_points += len(s.points)
        self.gated_refused += counts[1]
        return ev, gate, kept, counts, new

    def _remove(self, codes, ev):
        codes = np.asarray(codes, dtype=np.int64)
        live = np.unique(self.log_code)
        gone = np.intersect1d(live, codes)
        keep = ~np.isin(self.log_code, gone)
        self.log_p, self.log_c, self.log_k, self.log_code = self.log_p[keep], self.log_c[keep], self.log_k[keep], self.log_code[keep]
        self.tombstones += len(gone)
        for name, st in self.broken.items():
            if name != "tombstones" or ev.kind.startswith("carve"):
                st[1] += len(gone)
        if ev.kind == "carve_async":
            self.pending_carve += len(gone)
            self.levels_stale |= self.levels_current and len(gone) > 0
        ev.removed, ev.removed_codes = len(gone), set(gone.tolist())
        self._changed()
        return len(gone)

    def carve(self, kind, pose, params):
        """-> (event, the reference's Result on the model's keys, the removed keys sorted)."""
        ev = Event(kind)
        keys = self.keys
        res = mc.carve(keys, self.voxel, self.scan.points, pose, params)
        gone = keys[res.removed]
        self._remove(code_of(gone), ev)
        self.carve_rays += res.rays
        self.carve_removed += ev.removed
        return ev, res, mc.sorted_keys(gone)

    def evict(self, position, distance):
        """OracleMap.evict's rule on the model's map."""
        ev = Event("evict")
        before = self.keys
        om = self.oracle.OracleMap(self.voxel, self.cap)
        om.insert(self.log_p, self.log_c)
        removed = om.evict(position, distance)
        gone = np.setdiff1d(code_of(before), code_of(om.export()[0]))
        assert removed == len(gone)
        self._remove(gone, ev)
        return ev

    def erase(self, keys):
        ev = Event("erase")
        self._remove(code_of(keys), ev)
        return ev


def carve_params_of(draw):
    """The carve's parameters from the op's draw: min_hits 1 .. 3, stride 1 or 2, a margin of none or half a voxel."""
    d = int(draw * 12)
    return mc.Params(margin=(0.0, 0.25)[d % 2], max_range=60.0, min_hits=1 + (d // 2) % 3, stride=1 + d // 6)


def erased_tenth(keys, draw):
    """A tenth of the live keys, chosen by the op's draw."""
    n = len(keys)
    u = synth.rand_unit(int(draw * (1 << 30)), 920, np.arange(n, dtype=np.uint64))
    return np.ascontiguousarray(keys[np.argsort(u, kind="stable")[:max(1, n // 10)]])


# ---- the driver ------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Device:
    """A context and its twin (capi.Context both), and what the align reader compares with: conftest's pose_error and
    TIGHT_POSE_TOL, test_align_batch.py's assert_same_bits."""

    def __init__(self, capi, ctx, twin, pose_error, assert_same_bits, tight):
        self.capi, self.ctx, self.twin = capi, ctx, twin
        self.pose_error, self.assert_same_bits, self.tight = pose_error, assert_same_bits, tight


def run_walk(oracle, seed, raw, device=None, ops=None):
    """The walk of `seed` on the model, and on `device` (a Device) when there is one, every synchronous result and every
    reader compared.  -> (model, events, per full check the voxels of level 0 .. 3)."""
    ops = walk(seed, raw) if ops is None else ops
    scene = Scene(oracle, seed)
    model = Model(oracle, CAPS[seed % len(CAPS)])
    events, level_sizes, since, checks = [], [], [], [0]

    def checked(what, fn):
        checks[0] += 1
        try:
            fn()
        except Exception as e:                # a refusal of the library (VgicpError) names the walk too
            raise AssertionError(f"walk seed {seed} raw {raw}: check {checks[0]} ({what}) failed after the operations "
                                 f"{since} since the last full check that passed: {e}") from e

    for i, op in enumerate(ops):
        since.append((i, op))
        model.begin(op.kind)
        ev = apply(op, model, scene, device, checked)
        if ev is not None:
            events.append((i, ev))
        if op.kind.startswith("read_"):
            reader(op.kind[5:], model, device, checked)
            model.note_reader(op.kind[5:])
        if (i + 1) % FULL_CHECK_EVERY == 0 or i + 1 == len(ops):
            for name in READERS:
                if name != "points" or raw:
                    reader(name, model, device, checked)
                    model.note_reader(name)
            level_sizes.append([len(l) for l in model.level_list(3)])
            since = []
    model.checks = checks[0]                  # comparisons with the device that ran (0 without one)
    return model, events, level_sizes


def apply(op, model, scene, device, checked):
    """One update on the model and, with a device, on its context.  -> the model's Event, or None for a reader / a scan."""
    ctx = device.ctx if device else None
    kind = op.kind
    if kind == "reset":
        model.reset(VOXEL, 0)
        if ctx:
            ctx.map_reset(VOXEL, 0)
        return None
    if kind == "upload":
        s = scene.scan(op.scan, False)
        model.set_scan(s)
        if ctx:
            ctx.scan_upload(s.points, s.covs)
        return None
    if kind == "prepare":
        s = scene.scan(op.scan, True)
        model.set_scan(s)
        if ctx:
            kept, _ = ctx.scan_prepare(s.raw, None, None, None, PREP_VOXEL, KNN)
            gp, gc = ctx.scan_download()

            def prepared():
                assert kept == len(s.points) and same_bits(gp, s.points) and same_bits(gc, s.covs), "the prepared scan is not the oracle's"
            checked("scan_prepare", prepared)
        return None
    s = model.scan
    if kind == "insert_scan":
        own = scene.scan(op.scan, False)
        ev, new = model.insert(kind, own.points, own.covs, own.pose)
        if ctx:
            got = ctx.map_insert_scan(own.points, own.covs, own.pose, model.cap)
            checked(kind, lambda: _equal(got, new, "new voxels"))
        return ev
    if kind in ("insert_resident", "insert_resident_async"):
        ev, new = model.insert(kind, s.points, s.covs, s.pose)
        if ctx and kind == "insert_resident":
            got = ctx.map_insert_resident(s.pose, model.cap)
            checked(kind, lambda: _equal(got, new, "new voxels"))
        elif ctx:
            ctx.map_insert_resident_async(s.pose, model.cap)
        return ev
    if kind in ("gated", "gated_async"):
        ev, gate, kept, counts, new = model.gated(kind, s.pose)
        if ctx and kind == "gated":
            got_kept, st = ctx.map_insert_resident_gated(s.pose, model.cap, gate)

            def gated():
                assert np.array_equal(got_kept, kept), ("kept", int((got_kept != kept).sum()))
                _equal((st.points, st.matched, st.refused, st.not_finite, st.new_voxels), (len(kept),) + counts + (new,), "stats")
            checked(kind, gated)
        elif ctx:
            ctx.map_insert_resident_gated_async(s.pose, model.cap, gate)
        return ev
    if kind in ("carve", "carve_async"):
        params = carve_params_of(op.draw)
        ev, res, gone = model.carve(kind, s.pose, params)
        if ctx and kind == "carve":
            got_keys, st = ctx.map_carve_resident(s.pose, params.as_dict())

            def carved():
                assert np.array_equal(mc.sorted_keys(got_keys), gone), ("removed keys", len(got_keys), len(gone))
                _equal(dict(rays=st.rays, visits=st.visits, touched=st.touched, shielded=st.shielded, removed=st.removed),
                       res.counts(), "stats")
            checked(kind, carved)
        elif ctx:
            ctx.map_carve_resident_async(s.pose, params.as_dict())
        return ev
    if kind == "evict":
        position, distance = s.pose[:3, 3].copy(), EVICT_DISTANCES[int(op.draw * len(EVICT_DISTANCES))]
        ev = model.evict(position, distance)
        if ctx:
            got = ctx.map_evict(position, distance)
            checked(kind, lambda: _equal(got, ev.removed, "removed"))
        return ev
    if kind == "erase":
        victims = erased_tenth(model.keys, op.draw)
        ev = model.erase(victims)
        if ctx:
            ctx.map_erase(victims)
        return ev
    if kind == "levels":
        model.levels = int(op.draw * 4)
        if model.levels == 0:
            model.levels_current = model.levels_stale = False      # released
        model.note_reader("build")
        if ctx:
            built = ctx.map_levels_build(model.levels)
            want = model.level_list()
            checked(kind, lambda: _equal((built.levels, built.voxels[:model.levels + 1]), (model.levels, [len(l) for l in want]), "levels built"))
        return None
    assert kind.startswith("read_"), kind
    return None


def _equal(got, want, what):
    assert got == want, (what, got, want)


def reader(name, model, device, checked):
    """One reader of the device against the model (nothing to read without a device)."""
    if device is None:
        return
    ctx, capi = device.ctx, device.capi
    s = model.scan
    if name == "export":
        def export():
            got, want = ctx.map_export(), model.export()
            for what, g, w in zip(("keys", "means", "covs", "counts"), got, want):
                assert same_bits(g, w), (what, g.shape, w.shape)
        checked(name, export)
    elif name == "size":
        checked(name, lambda: _equal(ctx.map_size(), (model.voxels, model.slots), "(voxels, table_slots)"))
    elif name == "points":
        def points():
            from test_map_raw_points import grouped
            size, capacity = ctx.map_points_size()
            keys, pts = ctx.map_points_export()
            got, want = grouped(keys, pts), model.raw_lists()      # grouped: a voxel's points are contiguous
            assert size == len(pts) == sum(len(v) for v in want.values()) and capacity >= size, (size, len(pts), capacity)
            assert set(got) == set(want), (len(got), len(want))
            for k, w in want.items():
                assert same_bits(got[k], w), k
        checked(name, points)
    elif name == "levels":
        def levels():
            want = model.level_list()
            for l in range(1, model.levels + 1):
                got = ml.as_level(*ctx.map_level_export(l))
                assert ml.same_level(got, want[l]), (l, len(got), len(want[l]))
                voxels, slots, h = ctx.map_level_size(l)
                assert (voxels, slots, h) == (len(want[l]), next_pow2(max(MIN_SLOTS, 2 * model.voxels)), VOXEL * 2 ** l), (l, voxels, slots, h)
            assert ctx.map_level_size(0) == (model.voxels, model.slots, VOXEL)
        checked(name, levels)
    elif name == "align":
        def align():
            twin = device.twin
            keys, means, covs, _ = model.export()
            twin.map_reset(VOXEL, len(keys))
            twin.map_upsert(keys, means, covs)
            twin.scan_upload(s.points, s.covs)
            guess = s.pose @ synth.se3_to_SE3(ALIGN_OFFSET)
            ref = model.om.align(s.points, s.covs, guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS)
            for flags in (0, capi.FLAG_NO_PERSISTENT):
                got = ctx.align_resident(guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS, flags=flags)
                want = twin.align_resident(guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS, flags=flags)
                device.assert_same_bits(got, want, f"flags {flags}: the walked context against its twin")
                assert (got.launches == 1) == (flags == 0), (flags, got.launches)     # one persistent launch, or the loop
                assert got.iterations == ref.iterations == ALIGN_ROUNDS, (got.iterations, ref.iterations)
                assert np.array_equal(got.corr_count, ref.corr_count), (flags, got.corr_count, ref.corr_count)
                dt, dr = device.pose_error(got.pose, ref.pose)
                assert dt <= device.tight and dr <= device.tight, (flags, dt, dr)
        checked(name, align)
    elif name == "locate":
        def locate():
            want_levels = model.level_list()
            for level in sorted({0, model.levels}):
                h = VOXEL * 2 ** level
                bests, planes = mloc.locate(want_levels[level].keys, h, s.points, [s.pose], LOCATE_WINDOW)
                got = ctx.locate_resident(s.pose, level, LOCATE_WINDOW)
                assert np.array_equal(got.hits, planes), (level, got.hits, planes)
                b = got.best[0]
                _equal({k: b[k] for k in ("hits", "cell", "offset", "points", "skipped")}, bests[0].as_dict(), f"best of level {level}")
                assert same_bits(b["pose"], bests[0].pose), level
        checked(name, locate)
    elif name == "rays":
        def rays():
            want = mr.rays(model.keys, VOXEL, s.points, s.pose, RAY_PARAMS)
            got = ctx.rays_resident(s.pose, RAY_PARAMS.as_dict())
            _equal(got.counts[0], want.counts(), "counts")
            assert np.array_equal(got.status, want.status) and np.array_equal(got.steps, want.steps)
            assert np.array_equal(got.hit_key, want.hit_key)
            assert np.array_equal(got.range.view(np.uint64), want.range.view(np.uint64))
        checked(name, rays)
    elif name == "totals":
        def totals():
            _equal(ctx.map_gated_totals(), (model.gated_points, model.gated_refused), "gated totals")
            _equal(ctx.map_carve_totals(), (model.carve_rays, model.carve_removed), "carve totals")
        checked(name, totals)
    else:
        raise AssertionError(name)
