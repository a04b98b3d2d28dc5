"""The reference of the scan walks: ONE host model of the resident scan behind every entry point of the C ABI that makes,
replaces, consumes or reads it, the scene the walks run in, the walks themselves and the driver that holds a device context
against the model step by step.  Not a test module; tests/test_scan_walk_cpu.py checks the model against the references it is
made of and the committed seeds' conditions, tests/test_scan_walk.py drives the device.  The voxel map behind the deferred
consumers is map_walk_reference.Model, fed by this walk's insertions, gates and carves.

THE MODEL.  The resident scan is one of three things: none, settled (points, covariances, what vgicp_scan_info answers) or
pending (a preparation that was only enqueued: good, or refused — the refusal is reported by the first entry that settles,
which then does nothing else, and the scan is none from there on).  Around it the host's bookkeeping as include/vgicp_hip.h
states it: the generation counter as a relation (strictly greater after every operation that replaces the scan, the
refused ones included; unchanged otherwise), the fetch (open or not, checksums valid or not), the capacity of the scan's
device memory (n + n / 4, grow-only), the staged tickets (three slots, each ticket used once, numbered from 1 in the order
they are given out), the deferred consumer whose totals are still on the device and the copy they will travel with.  Every
expectation follows from the model and the headers, never from what a device returned — with ONE exception that the
header forces: the ORDER of a scan that vgicp_scan_from_map made is the source table's slot order, which no model knows;
the driver takes it from vgicp_scan_from_map_keys, checks that it is a permutation of the model's keys, and every byte is
compared from there on (without a device the order is the keys').

THE WALK.  A seeded shuffle of a multiset of FRAGMENTS — one operation, or the few operations in a row that one of the
conditions of tests/test_scan_walk_cpu.py names — packed into blocks of FULL_CHECK_EVERY operations with a seeded reader in
every remaining place, so that every kind occurs in every walk and the full check of every reader, which settles
everything, falls between fragments and never inside one.
"""
import json
import os
import sys
from dataclasses import dataclass

import numpy as np

if __name__ == "__main__":     # a walk in a process of its own (main below): the repository's root before the package is asked for
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import map_levels_reference as ml
import map_submap_reference as msub
import map_walk_reference as mw
from eskf_lio_amd import synth
from map_walk_reference import Model, same_bits

VOXEL, PREP_VOXEL, KNN = mw.VOXEL, mw.PREP_VOXEL, mw.KNN
FULL_CHECK_EVERY = 8
UPLOAD_RAW, UPLOAD_VOXEL = 4500, 0.1
# either side of the upload unit (2 048 points) and of a preparation tile (1 024), up and down in turn
UPLOAD_SIZES = (1500, 300, 2049, 1023, 3000, 700, 2047, 1025)
RAW_SIZES = (4000, 600, 2049, 1023, 6000, 1025, 3000, 2047)
SMALL_UPLOAD, FIRST_RAW = 300, 4000     # the prefix: 300 points (capacity 1 024), then a sweep of 4 000 (reallocation)
CAPS = mw.CAPS
SRC_LEVELS = 2
SRC_SCANS = 3
POSES = 6                              # scan k sits at the scene's pose k % POSES: every scan overlaps the map
EXTRINSIC_XI = (0.01, -0.02, 0.03, 0.002, -0.001, 0.003)
FAR = 1e9                              # one point beyond the search grid (+-2^17 voxel sizes), as tests/test_scan_fetch.py
ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS, ALIGN_OFFSET = mw.ALIGN_ROUNDS, mw.ALIGN_TSQ, mw.ALIGN_COS, mw.ALIGN_OFFSET
BATCH_OFFSET = (-0.03, 0.02, 0.01, -0.002, 0.003, 0.001)
RAY_PARAMS = mw.RAY_PARAMS
OK, BAD_ARGUMENT, NOT_READY = 0, 1, 7
COUNTER_FALLBACKS, COUNTER_GENERATION = 1, 5
# status and whole text, as the headers and the plans state them
REFUSED = (BAD_ARGUMENT, "a point lies beyond the search grid (more than 2^17 voxel sizes from the origin)")
UNBRACKETED = (BAD_ARGUMENT, "the IMU states do not bracket the end of the sweep")
NO_SCAN = (NOT_READY, "no scan resident: call vgicp_scan_upload first")                 # vgicp_resident_plan.h: kNoScanText
NO_SCAN_INFO = (NOT_READY, "no scan resident")
NO_SCAN_DOWNLOAD = (NOT_READY, "no scan resident: call vgicp_scan_upload or vgicp_scan_prepare first")
NO_SUMS = (NOT_READY, "no checksums: the last host copy did not come through vgicp_scan_fetch_begin / _end's kernel")
NO_KEYS = (NOT_READY, "the resident scan is not one that vgicp_scan_from_map made")
SLOTS_FULL = (NOT_READY, "three sweeps are staged ahead already: prepare one (or vgicp_sweep_unstage it) first")
NO_TICKET_PREPARE = (BAD_ARGUMENT, "no sweep staged under this ticket (staged by vgicp_sweep_stage, used once)")
NO_TICKET_UNSTAGE = (BAD_ARGUMENT, "no sweep staged under this ticket (used, dropped already, or never given out)")
NO_TIMES = (BAD_ARGUMENT, "the sweep was staged without capture times")
# The committed seeds: each meets the conditions of tests/test_scan_walk_cpu.py; found by running them over the seeds 1 .. 59
# (about one in four meets them all).  One cap each (CAPS[seed % 4]: 3, 5, 8, 20); each would see every break of ScanModel.BREAKS
SEEDS = (56, 1, 22, 11)

SOURCES = ("upload", "align_fused", "accumulate", "prepare", "prepare_async", "stage", "stage_cloud2", "from_map")
DEFERRED = ("insert_resident_async", "gated_async", "carve_async")
BYSTANDERS = ("preprocess", "deskew", "match", "voxel_index", "solve_step")
# readers that settle what is pending before they answer: a pending refusal surfaces in any of them
SETTLING = ("info", "download", "fetch_begin", "fetch_end", "align", "batch", "evaluate", "points", "rays")
# (the order of a full check: the fetch first, while a preparation may still be pending and the fetch kernel delivers it)
READERS = ("generation", "fetch", "fetch_sums", "info", "download", "keys", "align", "batch", "evaluate", "points", "rays", "map")
PREFIX = ("reset", "upload:small", "insert_resident", "insert_resident_async", "prepare_async:first", "read_info", "read_map")
# "R": a settling reader by the op's draw.  "kind:arg": the variant the conditions need.
FRAGMENTS = (
    # a refused preparation, the reader the refusal surfaces in, and recovery by each kind of source; both align paths read it
    ("prepare_async:refused", "R", "upload", "read_align"),
    ("prepare_async:refused", "R", "align_fused", "read_align"),
    ("prepare_async:refused", "R", "accumulate", "read_align"),
    ("prepare_async:refused", "R", "prepare", "read_align"),
    ("prepare_async:refused", "R", "prepare_async", "read_fetch_begin", "upload:same", "read_fetch_end", "read_fetch_sums"),
    ("stage", "prepare_async:refused", "R", "prepare_staged", "read_align"),         # staged before a replacement, prepared after
    ("stage_cloud2", "prepare_async:refused", "R", "prepare_staged", "read_align"),
    ("prepare_async:refused", "R", "from_map", "read_align"),
    # a fetch across a replacement
    ("prepare_async", "read_fetch_begin", "prepare_async:refused", "read_fetch_end"),
    ("prepare_async", "read_fetch_begin", "prepare_async", "read_fetch_end", "read_fetch_sums"),
    ("prepare_async", "read_fetch_begin", "align_fused", "read_fetch_end", "read_fetch_sums"),
    # a deferred consumer's totals in the next preparation's counter copy, settled by a reader that is not the map's
    ("upload", "insert_resident_async", "prepare_async", "read_info", "read_map"),
    ("prepare", "gated_async", "stage", "prepare_staged", "read_align", "read_map"),
    ("upload", "carve_async", "prepare_async", "read_info", "read_map"),
    ("prepare", "upload:small", "read_download"),                                      # the stale tail
    ("prepare_async", "prepare_async", "read_align"),                                  # the second replaces a pending scan
    ("read_info", "stage", "stage_cloud2", "stage", "stage", "unstage", "prepare_staged:dropped", "prepare_staged"),
    ("stage:notimes", "prepare_staged:states", "prepare_staged", "unstage:used"),
    ("prepare_async", "from_map:pending", "read_keys", "read_download"),
    ("from_map:empty", "R"),
    ("prepare:unbracketed", "R"),
    ("prepare_async:deskew", "preprocess", "read_info"),
    ("deskew",), ("match",), ("voxel_index",), ("solve_step",),
    ("insert_resident_async",), ("gated_async",), ("carve_async",),
    ("prepare_staged",), ("unstage",),
)
WALK_BLOCKS = 15
WALK_LENGTH = WALK_BLOCKS * FULL_CHECK_EVERY


# ---- the walk --------------------------------------------------------------------------------------------------------
@dataclass
class Op:
    kind: str
    arg: str = ""
    scan: int = -1            # a source's scan number within the walk
    draw: float = 0.0         # the op's own uniform draw in [0, 1)

    def __repr__(self):
        return self.kind + (":" + self.arg if self.arg else "") + (f"#{self.scan}" if self.scan >= 0 else "")


def walk(seed, raw):
    """The WALK_LENGTH operations of a walk: the prefix, then the fragments in a seeded order, packed first-fit into blocks
    of FULL_CHECK_EVERY operations, a seeded reader in every remaining place (between fragments, at seeded positions)."""
    idx = np.arange(4 * WALK_LENGTH, dtype=np.uint64)
    order = np.argsort(synth.rand_u64(seed, 931, idx[:len(FRAGMENTS)]), kind="stable")
    blocks = [[PREFIX]] + [[] for _ in range(WALK_BLOCKS - 1)]
    for f in (FRAGMENTS[i] for i in order):
        for b in blocks:
            if sum(len(g) for g in b) + len(f) <= FULL_CHECK_EVERY:
                b.append(f)
                break
        else:
            raise AssertionError(f"seed {seed}: the fragments do not fit {WALK_BLOCKS} blocks")
    pick = (synth.rand_unit(seed, 932, idx) * len(READERS)).astype(np.int64)
    place = synth.rand_unit(seed, 933, idx)
    names, r = [], 0
    for bi, b in enumerate(blocks):
        while sum(len(g) for g in b) < FULL_CHECK_EVERY:
            at = (1 if bi == 0 else 0) + int(place[r] * (len(b) + (0 if bi == 0 else 1)))     # never in front of the prefix
            b.insert(min(at, len(b)), ("read_" + READERS[pick[r]],))
            r += 1
        names += [n for g in b for n in g]
    assert len(names) == WALK_LENGTH
    draws = synth.rand_unit(seed, 934, idx[:WALK_LENGTH])
    ops, scans = [], 0
    for i, name in enumerate(names):
        kind, _, arg = name.partition(":")
        if kind == "R":
            kind = "read_" + SETTLING[int(draws[i] * len(SETTLING))]
        op = Op(kind, arg, draw=float(draws[i]))
        if kind in SOURCES or kind == "insert_resident":
            op.scan, scans = scans, scans + 1
        ops.append(op)
    return ops


# ---- the scene -------------------------------------------------------------------------------------------------------
@dataclass
class Sweep:
    raw: np.ndarray           # as the caller hands it over (a cloud2 sweep: the float32 values, widened)
    times: np.ndarray
    states: np.ndarray        # None: no deskew
    extrinsic: np.ndarray     # None: none
    scan: mw.Scan             # what the oracle chain makes of it; None for a refused one
    info: tuple = (0, 0, 0)   # what vgicp_scan_info must answer: (kept, deskewed, indefinite)

    def records(self):
        """The PointCloud2 payload of tests/test_scan_fetch.py: float32 x y z at 0 / 4 / 8, a float64 time at 16, 24 bytes."""
        n = len(self.raw)
        rec = np.zeros((n, 24), dtype=np.uint8)
        for c in range(3):
            rec[:, 4 * c:4 * c + 4] = self.raw[:, c].astype("<f4").view(np.uint8).reshape(n, 4)
        rec[:, 16:24] = self.times.astype("<f8").view(np.uint8).reshape(n, 8)
        return rec


class Scene(mw.Scene):
    """map_walk_reference's scene with scans of many sizes: scan k of a walk has UPLOAD_SIZES / RAW_SIZES[(seed + k) % 8]
    points, so successive scans differ in size in both directions."""

    def __init__(self, oracle, seed):
        super().__init__(oracle, seed)
        self.states = synth.make_imu_states(48, seed=5)
        self.ext = synth.se3_to_SE3(EXTRINSIC_XI)

    def _raw(self, n, k):
        raw = synth.make_lidar_scan(n, seed=self.seed * 1000 + k, extent=mw.EXTENT) - np.array([0.0, 0.0, mw.SENSOR_HEIGHT])
        return np.ascontiguousarray(raw)

    def at(self, k):
        return self.pose(k % POSES)

    def upload(self, k, n=None):
        """-> mw.Scan of n points: the first n kept points of a preparation at UPLOAD_VOXEL."""
        n = UPLOAD_SIZES[(self.seed + k) % len(UPLOAD_SIZES)] if n is None else n
        if ("u", k) not in self.cache:
            self.cache["u", k] = self.oracle.preprocess(self._raw(UPLOAD_RAW, k), UPLOAD_VOXEL, KNN)[:2]
        p, c = self.cache["u", k]
        assert 0 < n <= len(p), (n, len(p))
        return mw.Scan(np.ascontiguousarray(p[:n]), np.ascontiguousarray(c[:n]), self.at(k))

    def sweep(self, k, ext=False, deskew=False, cloud2=False, n=None, unbracketed=False):
        key = ("s", k, ext, deskew, cloud2, n, unbracketed)
        if key not in self.cache:
            n_raw = RAW_SIZES[(self.seed + k) % len(RAW_SIZES)] if n is None else n
            raw = self._raw(n_raw, k)
            if cloud2:
                raw = raw.astype(np.float32).astype(np.float64)           # what the device widens the wire floats to
            st = self.states
            times = synth.make_point_times(n_raw, st[1, 0] + 1e-4, st[-3, 0] + 0.4 / 400.0, seed=k)
            if unbracketed:
                times = times + 10.0                                       # no state after the end of the sweep
            pts = raw
            if ext:
                pts, _ = self.oracle.transform(pts, np.tile(np.eye(3).reshape(9), (n_raw, 1)), self.ext)
            done = 0
            if deskew or unbracketed:
                pts, done = self.oracle.deskew(pts, times, st)
                assert (done == -1) if unbracketed else (done > 0), done
            scan, info = None, (0, -1, 0)
            if not unbracketed:
                p, c, _, bad = self.oracle.preprocess_ex(pts, PREP_VOXEL, KNN)
                scan, info = mw.Scan(p, c, self.at(k), raw), (len(p), done if deskew else 0, bad)
            self.cache[key] = Sweep(raw, times, st if (deskew or unbracketed) else None, self.ext if ext else None, scan, info)
        return self.cache[key]

    def refused(self, k, ext, deskew):
        """The sweep with one point beyond the search grid."""
        good = self.sweep(k, ext, deskew)
        raw = good.raw.copy()
        raw[len(raw) // 2, 0] = FAR
        return Sweep(raw, good.times, good.states, good.extrinsic, None)


def variant(draw):
    """(extrinsic, deskew) of a preparation from the op's draw."""
    d = int(draw * 4)
    return bool(d & 1), bool(d & 2)


# ---- the model -------------------------------------------------------------------------------------------------------
@dataclass
class Resident:
    points: np.ndarray
    covs: np.ndarray
    pose: np.ndarray
    info: tuple               # what vgicp_scan_info answers
    source: str               # the kind of source that made it
    number: int               # the walk's operation that made it
    keys: np.ndarray = None   # a scan from a map: its voxels' keys and counts, in scan order
    counts: np.ndarray = None

    @property
    def n(self):
        return len(self.points)


@dataclass
class Ticket:
    number: int               # what the device gives out: 1, 2, ... in the order of the stagings that succeed
    sweep: Sweep
    has_times: bool
    cloud2: bool
    staged_at: int            # the scan generation (model's count of replacements) it was staged at


@dataclass
class Record:
    """What one operation did (tests/test_scan_walk_cpu.py's conditions are stated on these)."""
    i: int
    kind: str
    arg: str = ""
    error: tuple = None
    replaced: bool = False
    surfaced: bool = False    # a pending refusal was reported by this operation
    before: str = "none"      # the scan when the operation began: none, settled, pending, refused
    after: str = "none"
    n_before: int = 0
    n_after: int = 0
    source: str = ""          # the kind of source of the scan the operation read or made
    realloc: bool = False
    deferred_before: str = "" # the deferred consumer whose totals were still on the device when it began
    totals_via: str = ""      # where the totals this operation settled came from: prep, own
    fetch_open_before: bool = False
    fetched_n: int = 0        # kept count of the scan the open fetch was begun for
    ticket_age: int = 0       # prepare_staged: replacements since the ticket was staged
    note: str = ""
    map_event: object = None  # mw.Event of a deferred consumer


def state_of(m):
    return "refused" if m.pending == "refused" else "none" if m.scan is None else "pending" if m.pending else "settled"


class ScanModel:
    # BREAKS (tests/test_scan_walk_cpu.py asks that the committed walks together would see each):
    #   forget_fetch        begin_scan does not call forget_fetch: a fetch opened for the old scan, and its checksums, live on
    #   generation_upload / _prepare / _from_map   that caller of begin_scan does not advance the generation
    #   settle_scan         settle_scan leaves the refused scan as it was (n, scan_ready): with n alone kept no entry would
    #                       notice — every reader asks scan_ready first — so the break modelled is the wider one, and the
    #                       reader AFTER the one that reported the refusal is where it shows
    #   totals_from_own     settle_insert reads h_ins_counters although the totals travelled with a preparation's copy
    #   totals_from_prep    ... and the other way round
    #   used_ticket         a slot in state 2 (handed to the device) is found again under its ticket
    BREAKS = ("forget_fetch", "generation_upload", "generation_prepare", "generation_from_map", "settle_scan",
              "totals_from_own", "totals_from_prep", "used_ticket")

    def __init__(self, oracle, cap):
        self.oracle = oracle
        self.map, self.src = Model(oracle, cap), Model(oracle, cap)
        self.scan, self.pending = None, None          # pending: None, "good", "refused"
        self.replacements = 0
        self.capacity = 0
        self.fetch_open, self.fetch_for, self.sums_valid = False, None, False
        self.b_fetch_open, self.b_sums_valid = False, False     # as the library without forget_fetch keeps them
        self.tickets, self.used, self.given, self.busy = [], [], 0, 0
        self.deferred, self.deferred_via, self.deferred_changed = "", "", False
        self.keys_current = False
        self.stale_refusal = False
        self.map_version = 0
        self.records, self.rec = [], None
        self.seen = {b: False for b in self.BREAKS}

    # -- one operation --
    def begin(self, i, op):
        self.rec = Record(i, op.kind, op.arg, before=state_of(self), n_before=self.scan.n if self.scan is not None else 0,
                          deferred_before=self.deferred, fetch_open_before=self.fetch_open,
                          fetched_n=self.fetch_for.n if self.fetch_open and self.fetch_for is not None else 0,
                          source=self.scan.source if self.scan is not None else "")
        self.records.append(self.rec)
        self.map.begin(op.kind if op.kind in DEFERRED else "read")
        return self.rec

    def end(self):
        self.rec.after, self.rec.n_after = state_of(self), self.scan.n if self.scan is not None else 0

    def settle(self):
        """Everything deferred is brought up to date -> the refusal this reports, or None."""
        self.busy = 0
        if self.deferred:
            via = self.deferred_via or "own"
            self.rec.totals_via = via
            if self.deferred_changed:
                self.seen["totals_from_own" if via == "prep" else "totals_from_prep"] = True
            self.deferred, self.deferred_via, self.deferred_changed = "", "", False
        if self.stale_refusal:
            self.seen["settle_scan"] = True
        if self.pending == "refused":
            self.pending, self.stale_refusal = None, True
            self.rec.surfaced, self.rec.error = True, REFUSED
            return REFUSED
        self.pending = None
        return None

    def begin_scan(self, n_alloc, caller):
        """begin_scan of vgicp_capi_memory.inl: room for n_alloc points, the generation, the fetch."""
        if n_alloc > self.capacity:
            cap = max(n_alloc + n_alloc // 4, 1024)
            self.capacity, self.rec.realloc = (cap + 63) & ~63, self.capacity > 0
        self.replacements += 1
        self.rec.replaced = True
        self.seen["generation_" + caller] = True
        self.fetch_open = self.sums_valid = False
        self.scan, self.pending, self.keys_current, self.stale_refusal = None, None, False, False

    def enqueue_preparation(self):
        """A preparation's counter copy carries a pending consumer's totals when no copy has picked them up yet."""
        if self.deferred and not self.deferred_via:
            self.deferred_via = "prep"

    # -- sources --
    def upload(self, scan, source, settles=True):
        if settles and self.settle():
            return REFUSED
        self.begin_scan(scan.n if isinstance(scan, Resident) else len(scan.points), "upload")
        self.scan = Resident(scan.points, scan.covs, scan.pose, (len(scan.points), 0, 0), source, self.rec.i)
        self.rec.source = source
        return None

    def prepare(self, sweep, source, asynchronous, refused=False, unbracketed=False):
        if not asynchronous and self.settle():
            return REFUSED
        self.begin_scan(len(sweep.raw), "prepare")
        self.rec.source = source
        if unbracketed:
            self.rec.error = UNBRACKETED
            return UNBRACKETED
        self.enqueue_preparation()
        if refused:
            self.pending = "refused"
            if not asynchronous:
                return self.settle()
            return None
        s = sweep.scan
        self.scan = Resident(s.points, s.covs, s.pose, sweep.info, source, self.rec.i)
        self.pending = "good" if asynchronous else None
        if not asynchronous:
            self.settle()
        return None

    def stage(self, sweep, has_times, cloud2):
        """-> (error, the ticket's number)."""
        free = 3 - len(self.tickets) - self.busy
        if free <= 0:
            assert self.busy == 0, "a staging whose outcome depends on whether the device has finished: not a walk to commit"
            self.rec.error, self.rec.note = SLOTS_FULL, f"{len(self.tickets)} staged"
            return SLOTS_FULL, 0
        self.given += 1
        self.tickets.append(Ticket(self.given, sweep, has_times, cloud2, self.replacements))
        return None, self.given

    def present(self, which):
        """The ticket an operation presents -> (Ticket or None when it is not staged, its number)."""
        if which in ("dropped", "used") or not self.tickets:
            number = self.used[-1] if self.used else 0
            if number:
                self.seen["used_ticket"] = True
            return None, number
        return self.tickets[0], self.tickets[0].number

    def unstage(self, which):
        t, number = self.present(which)
        if t is None:
            self.rec.error = NO_TICKET_UNSTAGE
            return NO_TICKET_UNSTAGE, number
        self.tickets.remove(t)
        self.used.append(t.number)
        return None, number

    def prepare_staged(self, which, with_states):
        """-> (error, the ticket presented, its number)."""
        t, number = self.present(which)
        if t is None:
            self.rec.error = NO_TICKET_PREPARE
            return NO_TICKET_PREPARE, None, number
        if with_states and not t.has_times:
            self.rec.error, self.rec.note = NO_TIMES, "survives"
            return NO_TIMES, t, number
        self.tickets.remove(t)
        self.used.append(t.number)
        self.busy += 1
        self.rec.ticket_age = self.replacements - t.staged_at
        return self.prepare(t.sweep, "stage_cloud2" if t.cloud2 else "stage", True), t, number

    def from_map(self, sub, pose, order=None):
        """sub: msub.Submap of the source's level (sorted by key); order: the device's scan order as indices into it."""
        if self.settle():
            return REFUSED
        self.begin_scan(sub.voxels, "from_map")
        self.keys_current = True
        self.rec.source = "from_map"
        if len(sub) == 0:
            self.rec.note = "empty"
            return None
        order = np.arange(len(sub)) if order is None else order
        self.scan = Resident(np.ascontiguousarray(sub.points[order]), np.ascontiguousarray(sub.covs[order]), pose, (len(sub), 0, 0),
                             "from_map", self.rec.i, np.ascontiguousarray(sub.keys[order]), np.ascontiguousarray(sub.counts[order]))
        return None

    # -- deferred consumers --
    def consumer(self, kind, params=None):
        """-> (error, what the device is to be called with).  The verdict comes before the settling (vgicp_map_plan.h)."""
        if self.scan is None and self.pending is None:
            self.rec.error = NO_SCAN
            return NO_SCAN, None
        if (self.pending or self.deferred in ("insert_resident_async", "gated_async")) and self.settle():
            return REFUSED, None                      # settle_if_pending: a carve that is pending on its own is not waited for
        s = self.scan
        self.map.set_scan(mw.Scan(s.points, s.covs, s.pose))
        voxels, removed0 = self.map.voxels, self.map.carve_removed
        if kind == "insert_resident_async":
            ev, _ = self.map.insert(kind, s.points, s.covs, s.pose)
            out = None
        elif kind == "gated_async":
            ev, gate, _, _, _ = self.map.gated(kind, s.pose)
            out = gate
        else:
            ev, _, _ = self.map.carve(kind, s.pose, params)
            out = params
        self.map_version += 1
        self.rec.map_event, self.rec.source = ev, s.source
        changed = self.map.voxels != voxels or self.map.carve_removed != removed0 or ev.refused > 0
        if self.deferred and not self.deferred_via:   # a carve still pending: its totals and these go together
            changed |= self.deferred_changed
        self.deferred, self.deferred_via, self.deferred_changed = kind, "", changed
        return None, out

    # -- the fetch --
    def fetch_begin(self):
        """-> (error, kept)."""
        self.sums_valid = self.b_sums_valid = False
        if self.pending != "good":
            self.fetch_open = self.b_fetch_open = False
            err = self.settle()
            if err:
                return err, 0
            if self.scan is None:
                self.rec.error = NO_SCAN_INFO
                return NO_SCAN_INFO, 0
            return None, self.scan.n
        self.fetch_open = self.b_fetch_open = True
        self.fetch_for = self.scan
        return None, self.scan.n

    def fetch_end(self):
        """-> (error, the scan delivered)."""
        if self.b_fetch_open and not self.fetch_open:
            self.seen["forget_fetch"] = True          # the stale copy, or "two different sizes"
        through_kernel, self.fetch_open, self.b_fetch_open = self.fetch_open, False, False
        err = self.settle()
        if err:
            return err, None
        if self.scan is None:
            self.rec.error = NO_SCAN_DOWNLOAD if not through_kernel else NO_SCAN_INFO
            return self.rec.error, None
        self.sums_valid = self.b_sums_valid = through_kernel
        return None, self.scan

    def fetch_sums(self):
        if self.b_sums_valid and not self.sums_valid:
            self.seen["forget_fetch"] = True
        if not self.sums_valid:
            self.rec.error = NO_SUMS
            return NO_SUMS
        return None

    def reader(self, name):
        """A reader that settles, then needs a scan -> the error it must report, or None."""
        err = self.settle()
        if err:
            return err
        if self.scan is None:
            err = {"info": NO_SCAN_INFO, "download": NO_SCAN_DOWNLOAD}.get(name, NO_SCAN)
            self.rec.error = err
            return err
        self.rec.source = self.scan.source
        return None


def expected_sums(points, covs):
    """vgicp_scan_fetch_sums of the header on the model's bytes -> uint64[2][2][16]."""
    out = np.zeros((2, 2, 16), dtype=np.uint64)
    for arr, buf in enumerate((points, covs)):
        w = np.ascontiguousarray(buf).view(np.uint64).reshape(-1)
        idx = np.arange(len(w), dtype=np.uint64)
        for lane in range(16):
            wl = w[lane::16]
            with np.errstate(over="ignore"):
                out[arr, 0, lane] = wl.sum(dtype=np.uint64)
                out[arr, 1, lane] = ((np.uint64(len(wl)) - (idx[lane::16] >> np.uint64(4))) * wl).sum(dtype=np.uint64)
    return out


# ---- the driver ------------------------------------------------------------------------------------------------------
class Device(mw.Device):
    """map_walk_reference's Device (the walked context, its twin, conftest's pose_error and TIGHT_POSE_TOL,
    test_align_batch.py's assert_same_bits) with the source context of vgicp_scan_from_map and test_gpu_parity.py's
    _assert_fetch_sums."""

    def __init__(self, capi, ctx, twin, src, pose_error, assert_same_bits, tight, assert_fetch_sums):
        super().__init__(capi, ctx, twin, pose_error, assert_same_bits, tight)
        self.src, self.assert_fetch_sums = src, assert_fetch_sums


def error_of(e):
    return e.code, str(e).split(": ", 1)[1]


class Driver:
    """One walk on the model and, with a device (a Device with .src, the source context of vgicp_scan_from_map), on its
    context: every synchronous result, every refusal's status and whole text, and every reader compared."""

    def __init__(self, oracle, seed, raw, device=None):
        self.oracle, self.seed, self.raw, self.device = oracle, seed, raw, device
        self.scene = Scene(oracle, seed)
        self.model = ScanModel(oracle, CAPS[seed % len(CAPS)])
        self.ctx = device.ctx if device else None
        self.since, self.checks, self.implied = [], 0, 0     # comparisons made; comparisons the walk implies
        self.generation = 0
        self.twin_scan = self.twin_map = None
        self.numbers = {}          # the model's ticket number -> the device's

    # -- plumbing --
    def checked(self, what, fn):
        self.checks += 1
        try:
            return fn()
        except Exception as e:                # a refusal of the library (VgicpError) names the walk too
            raise AssertionError(f"scan walk seed {self.seed} raw {self.raw}: check {self.checks} ({what}) failed after the "
                                 f"operations {self.since} since the last full check that passed: {type(e).__name__}: {e}") from e

    def call(self, what, expect, fn, then=None):
        """fn on the device must raise `expect` (status, whole text) or, with None, succeed; then(result) compares."""
        self.implied += 1
        if self.ctx is None:
            return None

        def run():
            capi = self.device.capi
            try:
                out = fn()
            except capi.VgicpError as e:
                assert expect is not None and error_of(e) == tuple(expect), ("refused", error_of(e), "expected", expect)
                return None
            assert expect is None, ("succeeded, expected", expect)
            if then is not None:
                then(out)
            return out
        return self.checked(what, run)

    def check_generation(self, rec):
        """The relation, after every operation (the counter synchronises nothing)."""
        self.implied += 1
        if self.ctx is None:
            return

        def relation():
            now = self.ctx.counter(COUNTER_GENERATION)
            assert (now > self.generation) if rec.replaced else (now == self.generation), (rec.kind, rec.replaced, self.generation, now)
            self.generation = now
        self.checked("generation after " + rec.kind, relation)

    # -- the walk --
    def run(self, ops=None):
        ops = walk(self.seed, self.raw) if ops is None else ops
        for i, op in enumerate(ops):
            self.since.append((i, op))
            rec = self.model.begin(i, op)
            if op.kind.startswith("read_"):
                self.read(op.kind[5:], op)
            else:
                self.apply(op)
            self.model.end()
            self.check_generation(rec)
            if (i + 1) % FULL_CHECK_EVERY == 0 or i + 1 == len(ops):
                for name in READERS:
                    rec = self.model.begin(i, Op("full_" + name))
                    self.read(name, op)
                    self.model.end()
                    self.check_generation(rec)
                self.since = []
        self.model.checks, self.model.implied = self.checks, self.implied
        return self.model

    # -- updates --
    def apply(self, op):
        m, ctx, scene, kind = self.model, self.ctx, self.scene, op.kind
        ext, deskew = variant(op.draw)
        if kind == "reset":
            m.map.reset(VOXEL, 0)
            if ctx:
                ctx.map_reset(VOXEL, 0)
                self.build_source()
            else:
                self.build_source()
        elif kind == "upload":
            if op.arg == "same":              # as many points as the fetched scan kept, other bytes
                n = m.fetch_for.n if m.fetch_for is not None else SMALL_UPLOAD
                s = scene.upload(op.scan, min(n, 3000))
            else:
                s = scene.upload(op.scan, SMALL_UPLOAD if op.arg == "small" else None)
            err = m.upload(s, "upload")
            self.call(kind, err, lambda: ctx.scan_upload(s.points, s.covs))
        elif kind == "align_fused":
            s = scene.upload(op.scan)
            err = m.upload(s, "align_fused")
            guess = s.pose @ synth.se3_to_SE3(ALIGN_OFFSET)
            self.call(kind, err, lambda: ctx.align(s.points, s.covs, guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS, allow_degenerate=True),
                      lambda got: self.same_align(got, s, guess, fused=True))
        elif kind == "accumulate":
            s = scene.upload(op.scan)
            err = m.upload(s, "accumulate")
            self.call(kind, err, lambda: ctx.accumulate(s.points, s.covs, s.pose), lambda got: self.same_accumulate(got, s))
        elif kind == "insert_resident":       # the prefix: the map's first points (synchronous)
            s = m.scan
            m.map.set_scan(mw.Scan(s.points, s.covs, s.pose))
            _, new = m.map.insert(kind, s.points, s.covs, s.pose)
            m.map_version += 1
            self.call(kind, None, lambda: ctx.map_insert_resident(s.pose, m.map.cap), lambda got: _equal(got, new, "new voxels"))
        elif kind == "prepare":
            sw = scene.sweep(op.scan, ext, deskew, unbracketed=op.arg == "unbracketed")
            err = m.prepare(sw, "prepare", False, unbracketed=op.arg == "unbracketed")
            m.rec.note = "deskewed" if sw.info[1] > 0 else ""
            self.call(kind, err, lambda: ctx.scan_prepare(sw.raw, sw.times if sw.states is not None else None, sw.states, sw.extrinsic,
                                                          PREP_VOXEL, KNN), lambda got: _equal(got, sw.info[:2], "(kept, deskewed)"))
        elif kind == "prepare_async":
            if op.arg == "first":
                sw = scene.sweep(op.scan, False, False, n=FIRST_RAW)
            elif op.arg == "refused":
                sw = scene.refused(op.scan, ext, deskew)
            else:
                sw = scene.sweep(op.scan, ext, deskew or op.arg == "deskew")
            err = m.prepare(sw, "prepare_async", True, refused=op.arg == "refused")
            m.rec.note = "deskewed" if sw.info[1] > 0 else ""
            self.call(kind, err, lambda: ctx.scan_prepare_async(sw.raw, sw.times if sw.states is not None else None, sw.states,
                                                                sw.extrinsic, PREP_VOXEL, KNN))
        elif kind in ("stage", "stage_cloud2"):
            cloud2 = kind == "stage_cloud2"
            has_times = op.arg != "notimes"
            # the preparation's variant belongs to the ticket: what prepare_staged will be asked for
            sw = scene.sweep(op.scan, ext, deskew and has_times, cloud2=cloud2)
            err, number = m.stage(sw, has_times, cloud2)
            if cloud2:
                got = self.call(kind, err, lambda: ctx.sweep_stage_cloud2(sw.records(), len(sw.raw), 24, 0, 4, 8, 16))
            else:
                got = self.call(kind, err, lambda: ctx.sweep_stage(sw.raw, sw.times if has_times else None))
            if err is None:
                self.implied += 1
                if ctx:
                    self.checked("ticket", lambda: _equal(got, number, "ticket"))
        elif kind == "unstage":
            err, number = m.unstage(op.arg)
            self.call(kind, err, lambda: ctx.sweep_unstage(number))
        elif kind == "prepare_staged":
            err, t, number = m.prepare_staged(op.arg, op.arg == "states")
            sw = t.sweep if t is not None else None
            states = self.scene.states if op.arg == "states" else (sw.states if sw is not None else None)
            self.call(kind, err, lambda: ctx.scan_prepare_staged_async(number, states, sw.extrinsic if sw is not None else None,
                                                                       PREP_VOXEL, KNN))
        elif kind == "from_map":
            self.from_map(op)
        elif kind in DEFERRED:
            params = mw.carve_params_of(op.draw) if kind == "carve_async" else None
            err, out = m.consumer(kind, params)
            pose = m.scan.pose if m.scan is not None else np.eye(4)
            if kind == "insert_resident_async":
                self.call(kind, err, lambda: ctx.map_insert_resident_async(pose, m.map.cap))
            elif kind == "gated_async":
                self.call(kind, err, lambda: ctx.map_insert_resident_gated_async(pose, m.map.cap, out if out is not None else 1.0))
            else:
                self.call(kind, err, lambda: ctx.map_carve_resident_async(pose, params.as_dict()))
        elif kind in BYSTANDERS:
            self.bystander(op)
        else:
            raise AssertionError(kind)

    def build_source(self):
        """The source context of vgicp_scan_from_map: a map of SRC_SCANS scans of its own, SRC_LEVELS levels."""
        m = self.model
        m.src.reset(VOXEL, 0)
        src = self.device.src if self.device else None
        if src:
            src.map_reset(VOXEL, 0)
        for k in range(SRC_SCANS):
            s = self.scene.upload(900 + k, 1500)
            s.pose = self.scene.pose(k)
            m.src.insert("insert_scan", s.points, s.covs, s.pose)
            if src:
                src.map_insert_scan(s.points, s.covs, s.pose, m.src.cap)
        m.src.levels = SRC_LEVELS
        if src:
            src.map_levels_build(SRC_LEVELS)

    def from_map(self, op):
        m, ctx = self.model, self.ctx
        src = self.device.src if self.device else None
        pose = self.scene.at(op.scan)
        d = int(op.draw * 12)
        level, min_count, radius = d % 3, (0, 2)[(d // 3) % 2], (5.0, 8.0)[d // 6]
        center = pose[:3, 3].copy()
        if op.arg == "empty":
            center, radius = np.array([1000.0, 0.0, 0.0]), 1.0
        if op.arg == "pending":               # the source has an insertion pending when it is read
            s = self.scene.upload(950 + op.scan, 700)
            s.pose = self.scene.at(op.scan + 3)
            m.src.insert("insert_resident_async", s.points, s.covs, s.pose)
            if src:
                src.scan_upload(s.points, s.covs)
                src.map_insert_resident_async(s.pose, m.src.cap)
        frame = synth.invert_pose(pose)
        lv = ml.levels_of(*m.src.export(), SRC_LEVELS)[level]
        sub = msub.submap(lv.keys, lv.means, lv.covs, lv.counts, VOXEL * 2 ** level, center, radius, frame, min_count)
        assert (len(sub) == 0) == (op.arg == "empty"), (op, len(sub))
        refused = m.pending == "refused"
        got = self.call("from_map", REFUSED if refused else None,
                        lambda: ctx.scan_from_map(src, center, radius, frame, min_count=min_count, level=level),
                        lambda st: _equal((st.voxels, st.points, st.too_far, st.too_few), (sub.voxels, len(sub), sub.too_far, sub.too_few), "stats"))
        order = None
        if not refused and len(sub):
            self.implied += 1
        if got is not None and len(sub):
            def permutation():
                keys, counts = ctx.scan_from_map_keys()
                codes, want = mw.code_of(keys), mw.code_of(sub.keys)
                assert len(codes) == len(want) and np.array_equal(np.sort(codes), want), "the scan's keys are not the selected voxels'"
                o = np.searchsorted(want, codes)
                assert np.array_equal(counts, sub.counts[o]), "counts"
                return o
            order = self.checked("from_map order", permutation)
        err = m.from_map(sub, pose, order)
        assert (err is not None) == refused

    def bystander(self, op):
        """Each leaves scan, info and generation as they were (the next readers hold that); its own answer is the oracle's."""
        m, ctx, kind, o = self.model, self.ctx, op.kind, self.oracle
        err = m.settle() if kind != "solve_step" else None
        sw = self.scene.sweep(990, n=1025)
        if kind == "preprocess":
            want = o.preprocess(sw.raw, 0.4, KNN)
            self.call(kind, err, lambda: ctx.preprocess(sw.raw, 0.4, KNN),
                      lambda got: _bits(got[:2], want[:2], "preprocess") or _equal(list(got[2]), list(want[2]), "index"))
        elif kind == "deskew":
            want = o.deskew(sw.raw, sw.times, self.scene.states)
            self.call(kind, err, lambda: ctx.deskew(sw.raw, sw.times, self.scene.states),
                      lambda got: _bits(got[:1], want[:1], "deskew") or _equal(got[1], want[1], "moved"))
        elif kind == "voxel_index":
            want = o.voxel_index(VOXEL, sw.raw)
            self.call(kind, err, lambda: ctx.voxel_index(sw.raw), lambda got: _bits((got,), (want,), "keys"))
        elif kind == "match":
            s = self.scene.upload(991, 700)
            wp, wc = o.transform(s.points, s.covs, s.pose)
            want = m.map.om.match(wp, wc)
            self.call(kind, err, lambda: ctx.match(wp, wc), lambda got: _bits(got, want, "match"))
        else:
            A = np.diag([4.0, 5.0, 6.0, 7.0, 8.0, 9.0]) + 0.1
            b = np.array([0.1, -0.2, 0.3, 0.01, -0.02, 0.03])
            self.call(kind, err, lambda: ctx.solve_step(A, b))     # (tests/test_solver_domain.py holds what it answers)

    # -- what a source returns --
    def twin(self):
        """The twin context, brought to the model's map and handed the model's scan by scan_upload."""
        t, m = self.device.twin, self.model
        if self.twin_map != m.map_version:
            keys, means, covs, _ = m.map.export()
            t.map_reset(VOXEL, len(keys))
            t.map_upsert(keys, means, covs)
            self.twin_map = m.map_version
        if self.twin_scan is not m.scan:
            t.scan_upload(m.scan.points, m.scan.covs)
            self.twin_scan = m.scan
        return t

    def same_align(self, got, s, guess, flags=0, fused=False):
        ref = self.model.map.om.align(s.points, s.covs, guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS)
        t = self.twin()
        if fused:                                  # like with like: the twin's own vgicp_align of the host scan
            want = t.align(s.points, s.covs, guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS, allow_degenerate=True)
        else:
            want = t.align_resident(guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS, flags=flags, allow_degenerate=True)
        self.device.assert_same_bits(got, want, f"flags {flags}: the walked context against its twin")
        assert got.iterations == ref.iterations == ALIGN_ROUNDS, (got.iterations, ref.iterations)
        assert np.array_equal(got.corr_count, ref.corr_count), (flags, got.corr_count, ref.corr_count)
        assert got.status == 0 and got.corr_count.min() > 0, (got.status, got.corr_count)
        dt, dr = self.device.pose_error(got.pose, ref.pose)
        assert dt <= self.device.tight and dr <= self.device.tight, (flags, dt, dr)

    def same_accumulate(self, got, s):
        t = self.device.twin
        self.twin()                                # the map; the twin's own accumulate uploads the scan
        want = t.accumulate(s.points, s.covs, s.pose)
        self.twin_scan = None
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], "accumulate against the twin"
        wp, wc = self.oracle.transform(s.points, s.covs, s.pose)
        assert got[2] == self.model.map.om.accumulate(wp, wc)[2], "matched points against the oracle"

    # -- readers --
    def read(self, name, op):
        m, ctx = self.model, self.ctx
        capi = self.device.capi if self.device else None
        if name == "generation":
            return                             # held after every operation
        if name == "info":
            err = m.reader(name)
            self.call(name, err, ctx.scan_info if ctx else None, lambda got: _equal(got, m.scan.info, "(kept, deskewed, indefinite)"))
        elif name == "download":
            err = m.reader(name)
            self.call(name, err, ctx.scan_download if ctx else None, lambda got: _bits(got, (m.scan.points, m.scan.covs), "the resident scan"))
        elif name == "fetch_begin":
            err, kept = m.fetch_begin()
            self.call(name, err, ctx.scan_fetch_begin if ctx else None, lambda got: _equal(got, kept, "kept"))
        elif name == "fetch_end":
            capacity = max(m.scan.n if m.scan is not None else 0, m.rec.fetched_n, 1)
            err, s = m.fetch_end()
            self.call(name, err, lambda: ctx.scan_fetch_end(capacity), lambda got: _bits(got, (s.points, s.covs), "the scan resident when it is called"))
        elif name == "fetch":
            err, kept = m.fetch_begin()
            self.call("fetch_begin", err, ctx.scan_fetch_begin if ctx else None, lambda got: _equal(got, kept, "kept"))
            err, s = m.fetch_end()
            self.call("fetch_end", err, lambda: ctx.scan_fetch_end(max(kept, 1)), lambda got: _bits(got, (s.points, s.covs), "the fetched scan"))
        elif name == "fetch_sums":
            err = m.fetch_sums()
            self.call(name, err, ctx.scan_fetch_sums if ctx else None,
                      lambda got: self.device.assert_fetch_sums(got, m.scan.points, m.scan.covs, "fetch_sums"))
        elif name == "keys":
            ok = m.keys_current
            if not ok:
                m.rec.error = NO_KEYS
            s = m.scan

            def same_keys(got):
                want = (s.keys, s.counts) if s is not None else (np.zeros((0, 3), np.int32), np.zeros(0, np.uint64))
                _bits(got, want, "keys and counts")
            self.call(name, None if ok else NO_KEYS, ctx.scan_from_map_keys if ctx else None, same_keys)
        elif name == "align":
            err = m.reader(name)
            s = m.scan
            guess = (s.pose if s is not None else np.eye(4)) @ synth.se3_to_SE3(ALIGN_OFFSET)
            if s is not None and err is None:       # what the seed's condition asks: every align has something to align to
                cc = m.map.om.align(s.points, s.covs, guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS).corr_count
                m.rec.note = str(int(cc.min()) if len(cc) == ALIGN_ROUNDS else 0)
            for flags in (0, capi.FLAG_NO_PERSISTENT) if capi else (0, 2):
                def aligned(got, flags=flags):
                    self.same_align(got, s, guess, flags)
                    assert (got.launches == 1) == (flags == 0), (flags, got.launches)     # one persistent launch, or the loop
                self.call(f"align flags {flags}", err, lambda: ctx.align_resident(guess, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS, flags=flags,
                                                                                  allow_degenerate=True), aligned)
                err = NO_SCAN if err is not None else None           # the refusal surfaced in the first: none from there on
        elif name == "batch":
            err = m.reader(name)
            base = m.scan.pose if m.scan is not None else np.eye(4)
            guesses = [base @ synth.se3_to_SE3(ALIGN_OFFSET), base @ synth.se3_to_SE3(BATCH_OFFSET)]

            def batch(got):
                want = self.twin().align_resident_batch(guesses, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS)
                assert len(got) == len(want) == 2
                for g, w in zip(got, want):
                    self.device.assert_same_bits(g, w, "batch against the twin")
            self.call(name, err, lambda: ctx.align_resident_batch(guesses, ALIGN_ROUNDS, ALIGN_TSQ, ALIGN_COS), batch)
        elif name == "evaluate":
            err = m.reader(name)
            base = m.scan.pose if m.scan is not None else np.eye(4)
            poses = [base, base @ synth.se3_to_SE3(ALIGN_OFFSET)]

            def evaluate(got):
                want = self.twin().evaluate_resident(poses)
                for g, w in zip(got, want):
                    assert (g.points, g.correspondences) == (w.points, w.correspondences) and g.points == m.scan.n
                    assert same_bits(np.array([g.cost, g.sq_error]), np.array([w.cost, w.sq_error])) and same_bits(g.normal_eq, w.normal_eq)
            self.call(name, err, lambda: ctx.evaluate_resident(poses), evaluate)
        elif name == "points":
            err = m.reader(name)
            some = m.scan is not None              # with no scan the arrays are not asked for: the entry's own refusal
            pose = m.scan.pose if some else np.eye(4)

            def points(got):
                want = self.twin().points_resident(pose, (0.5,))
                assert (got.points, got.matched, got.counted) == (want.points, want.matched, want.counted) and got.points == m.scan.n
                _bits((got.d2, got.sq_error, got.weight, got.status, got.quantiles), (want.d2, want.sq_error, want.weight, want.status, want.quantiles), "planes")
            self.call(name, err, lambda: ctx.points_resident(pose, (0.5,), d2=some, sq_error=some, weight=some, status=some), points)
        elif name == "rays":
            err = m.reader(name)
            some = m.scan is not None
            pose = m.scan.pose if some else np.eye(4)

            def rays(got):
                want = self.twin().rays_resident(pose, RAY_PARAMS.as_dict())
                _equal(got.counts, want.counts, "counts")
                _bits((got.status, got.steps, got.hit_key, got.range), (want.status, want.steps, want.hit_key, want.range), "planes")
            self.call(name, err, lambda: ctx.rays_resident(pose, RAY_PARAMS.as_dict(), per_point=some), rays)
        elif name == "map":
            err = m.settle()
            self.call("map size", err, ctx.map_size if ctx else None, lambda got: _equal(got, (m.map.voxels, m.map.slots), "(voxels, table_slots)"))
            for what in ("export", "totals") + (("points",) if self.raw else ()):
                self.implied += 1
                if ctx:
                    mw.reader(what, m.map, self.device, self.checked)
        else:
            raise AssertionError(name)


def _equal(got, want, what):
    assert got == want, (what, got, want)


def _bits(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w)), (what, k, np.shape(g), np.shape(w))


def run_walk(oracle, seed, raw, device=None, ops=None):
    """The walk of `seed` on the model, and on `device` when there is one.  -> the model (records, seen, checks)."""
    return Driver(oracle, seed, raw, device).run(ops)


def main(argv):
    """A walk in a process of its own (VGICP_STAGE_LIMIT is read once per process): prints one JSON line."""
    import test_scan_walk as tw
    from oracle import binding
    binding.load()
    seed, raw = int(argv[1]), argv[2] == "raw"
    model, fallbacks = tw.run(binding, None, seed, raw, upload_in_place=True)
    print(json.dumps({"stage_limit": os.environ.get("VGICP_STAGE_LIMIT"), "checks": model.checks, "implied": model.implied,
                      "fallbacks": list(fallbacks)}), flush=True)


if __name__ == "__main__":
    main(sys.argv)
