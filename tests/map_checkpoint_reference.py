"""The map checkpoint's blob (include/vgicp_hip_map_checkpoint.h, format 1) restated in numpy: pack(), parse(), checksum()
and check(), the fourteen rules in the header's order.  No device, no library: tests/test_map_checkpoint_cpu.py holds it
against hand-made blobs and against the plan header's check (tests/native/checkpoint_plan.cpp), tests/test_map_checkpoint.py
against what the device packs."""
import math
from dataclasses import dataclass

import numpy as np

MAGIC = b"VGICPMAP"
FORMAT, HEADER, RECORD, FLAG_RAW = 1, 128, 128, 1
MIN_SLOTS, MAX_SLOTS, RAW_MAX = 1024, 1 << 32, 1 << 31
SLOT_FULL = 1
RECORD_DTYPE = np.dtype([("key", "<i4", 3), ("state", "<i4"), ("mean", "<f8", 3), ("cov", "<f8", 9), ("count", "<u8"),
                         ("spare", "<u8")])
assert RECORD_DTYPE.itemsize == RECORD
HEADER_DTYPE = np.dtype([("magic", "S8"), ("format", "<u4"), ("header_bytes", "<u4"), ("total_bytes", "<u8"),
                         ("voxel_size", "<f8"), ("slots", "<u8"), ("voxels", "<u8"), ("tombstones", "<u8"),
                         ("raw_points", "<u8"), ("flags", "<u4"), ("record_bytes", "<u4"), ("checksum", "<u8"),
                         ("reserved", "u1", 48)])
assert HEADER_DTYPE.itemsize == HEADER


def pad8(v):
    return (v + 7) & ~7


def layout(F, T, P):
    """Byte offsets of the four sections and the total."""
    full_at = HEADER
    tomb_at = full_at + pad8(4 * F)
    records_at = tomb_at + pad8(4 * T)
    raw_at = records_at + RECORD * F
    return full_at, tomb_at, records_at, raw_at, raw_at + 24 * P


def total_bytes(F, T, P):
    return 128 + pad8(4 * F) + pad8(4 * T) + 128 * F + 24 * P


def checksum(payload) -> int:
    """Word i of the payload (as u64) times 2 i + 1, summed mod 2^64."""
    w = np.frombuffer(bytes(payload), dtype="<u8")
    with np.errstate(over="ignore"):
        return int((w * (2 * np.arange(len(w), dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


def records_of(keys, means, covs, counts):
    r = np.zeros(len(keys), dtype=RECORD_DTYPE)
    r["key"], r["state"], r["mean"], r["cov"], r["count"] = keys, SLOT_FULL, means, covs, counts
    return r


def pack(voxel_size, slots, full_slots, records, tomb_slots=(), raw=None) -> bytes:
    """A blob from its parts: full_slots (ascending) with their records, tomb_slots (ascending), raw: None (the map keeps
    no raw points) or P x 3 doubles in canonical order."""
    full_slots = np.asarray(full_slots, dtype="<u4")
    tomb_slots = np.asarray(tomb_slots, dtype="<u4")
    records = np.asarray(records, dtype=RECORD_DTYPE)
    F, T = len(full_slots), len(tomb_slots)
    P = 0 if raw is None else len(raw)
    full_at, tomb_at, records_at, raw_at, total = layout(F, T, P)
    out = bytearray(total)
    out[full_at:full_at + 4 * F] = full_slots.tobytes()
    out[tomb_at:tomb_at + 4 * T] = tomb_slots.tobytes()
    out[records_at:records_at + RECORD * F] = records.tobytes()
    if P:
        out[raw_at:total] = np.ascontiguousarray(raw, dtype="<f8").tobytes()
    h = np.zeros(1, dtype=HEADER_DTYPE)
    h["magic"], h["format"], h["header_bytes"], h["total_bytes"], h["voxel_size"] = MAGIC, FORMAT, HEADER, total, voxel_size
    h["slots"], h["voxels"], h["tombstones"], h["raw_points"] = slots, F, T, P
    h["flags"], h["record_bytes"], h["checksum"] = (FLAG_RAW if raw is not None else 0), RECORD, checksum(out[HEADER:])
    out[:HEADER] = h.tobytes()
    return bytes(out)


@dataclass
class Blob:
    header: dict
    full_slots: np.ndarray
    tomb_slots: np.ndarray
    records: np.ndarray      # RECORD_DTYPE
    raw: np.ndarray          # P x 3

    @property
    def raw_on(self):
        return bool(self.header["flags"] & FLAG_RAW)

    def raw_of_record(self):
        """Per record j its points (count x 3), by the exclusive prefix sum of the counts in record order."""
        ends = np.cumsum(self.records["count"].astype(np.int64))
        return [self.raw[e - c:e] for e, c in zip(ends, self.records["count"].astype(np.int64))]


def header_of(blob) -> dict:
    h = np.frombuffer(bytes(blob[:HEADER]), dtype=HEADER_DTYPE)[0]
    return {name: (h[name].tolist() if name != "reserved" else bytes(h[name])) for name in HEADER_DTYPE.names}


def parse(blob) -> Blob:
    """The sections of a blob that check() passes."""
    blob = bytes(blob)
    h = header_of(blob)
    F, T, P = h["voxels"], h["tombstones"], h["raw_points"]
    full_at, tomb_at, records_at, raw_at, total = layout(F, T, P)
    return Blob(h, np.frombuffer(blob, "<u4", F, full_at), np.frombuffer(blob, "<u4", T, tomb_at),
                np.frombuffer(blob, RECORD_DTYPE, F, records_at), np.frombuffer(blob, "<f8", 3 * P, raw_at).reshape(P, 3))


def check(blob) -> int:
    """0 when the blob passes, else the number of the first rule of the header's list that it fails."""
    blob = bytes(blob)
    if len(blob) < HEADER or blob[:8] != MAGIC:
        return 1
    h = header_of(blob)
    if (h["format"], h["header_bytes"], h["record_bytes"]) != (FORMAT, HEADER, RECORD):
        return 2
    if any(h["reserved"]) or h["flags"] & ~FLAG_RAW:
        return 3
    if not (math.isfinite(h["voxel_size"]) and h["voxel_size"] > 0.0):
        return 4
    slots, F, T, P = h["slots"], h["voxels"], h["tombstones"], h["raw_points"]
    if not MIN_SLOTS <= slots <= MAX_SLOTS or slots & (slots - 1):
        return 5
    if 2 * (F + T) > slots:
        return 6
    raw = bool(h["flags"] & FLAG_RAW)
    if (not raw and P != 0) or P > RAW_MAX:
        return 7
    if not len(blob) == h["total_bytes"] == total_bytes(F, T, P):
        return 8
    if checksum(blob[HEADER:]) != h["checksum"]:
        return 9
    b = parse(blob)
    full, tomb = b.full_slots.astype(np.int64), b.tomb_slots.astype(np.int64)
    if (full >= slots).any() or (np.diff(full) <= 0).any():
        return 10
    if (tomb >= slots).any() or (np.diff(tomb) <= 0).any():
        return 11
    if len(np.intersect1d(full, tomb)):
        return 12
    r = b.records
    if (r["state"] != SLOT_FULL).any() or (r["spare"] != 0).any() or (r["count"] < 1).any():
        return 13
    if raw and sum(int(c) for c in r["count"]) != P:
        return 14
    return 0
