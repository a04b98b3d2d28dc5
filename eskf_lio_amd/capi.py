"""ctypes binding of the C ABI in include/vgicp_hip.h (libvgicp_hip.so).

This is plumbing for tests and bench.py: it adds no compute and no fallback.  If the HIP module has
not been built, importing the library raises; if there is no gfx950 device, `Context()` raises
`VgicpError` carrying the library's message.  Nothing here imports the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VGICP_LIB_PATH: a developer's A/B aid (two builds of the module timed in one session on one box)
LIB_PATH = os.environ.get("VGICP_LIB_PATH") or os.path.join(_HERE, "lib", "libvgicp_hip.so")

OK, ERR_BAD_ARGUMENT, ERR_HIP, ERR_RCCL, ERR_TABLE_FULL, ERR_DEGENERATE, ERR_NO_DEVICE, ERR_NOT_READY, ERR_TIMEOUT = range(9)
FLAG_PROFILE = 1
FLAG_NO_PERSISTENT = 2
SOLVE_FORCE_PIVOTED = 1
UNIQUE_ID_BYTES = 128
PEER_HANDLE_BYTES = 64

# every symbol include/vgicp_hip.h declares
EXPORTS = (
    "vgicp_abi_version", "vgicp_create", "vgicp_create_multi", "vgicp_destroy", "vgicp_last_error", "vgicp_device_info",
    "vgicp_get_counter",
    "vgicp_map_reset", "vgicp_map_upsert", "vgicp_map_erase", "vgicp_map_size",
    "vgicp_map_insert_scan", "vgicp_map_insert_resident", "vgicp_map_evict", "vgicp_map_export",
    "vgicp_align", "vgicp_scan_upload", "vgicp_align_resident",
    "vgicp_accumulate", "vgicp_solve_step", "vgicp_match", "vgicp_voxel_index", "vgicp_preprocess", "vgicp_deskew",
    "vgicp_scan_prepare", "vgicp_scan_download",
    "vgicp_peer_status", "vgicp_scan_prepare_async", "vgicp_sweep_stage", "vgicp_sweep_stage_cloud2", "vgicp_sweep_unstage", "vgicp_scan_fetch_begin", "vgicp_scan_fetch_end", "vgicp_scan_fetch_sums", "vgicp_scan_prepare_staged_async", "vgicp_scan_info", "vgicp_map_insert_resident_async", "vgicp_get_frame_stats",
    "vgicp_set_option", "vgicp_host_register", "vgicp_host_unregister",
    "vgicp_comm_unique_id", "vgicp_comm_init", "vgicp_comm_destroy",
    "vgicp_peer_export", "vgicp_peer_connect", "vgicp_peer_disconnect",
)

# every symbol include/vgicp_hip_map_points.h declares (an extension header: EXPORTS stays the main header's list)
MAP_POINTS_EXPORTS = ("vgicp_map_points_size", "vgicp_map_points_export")

# every symbol include/vgicp_hip_batch.h declares (likewise an extension header)
BATCH_EXPORTS = ("vgicp_align_resident_batch", "vgicp_align_batch_width")
BATCH_MAX = 64

# every symbol include/vgicp_hip_evaluate.h declares (likewise an extension header)
EVALUATE_EXPORTS = ("vgicp_evaluate_resident",)
EVAL_MAX = 64

# The entry points of the later extension headers live in small libraries of their own beside the module, so that
# libvgicp_hip.so exports exactly the lists above: include/vgicp_hip_<name>.h is libvgicp_hip_<name>.so (side_lib_path),
# for every name of SIDE_EXPORTS (csrc/Makefile's SIDE).  Each tuple: every symbol its header declares
PRIOR_EXPORTS = ("vgicp_set_pose_prior", "vgicp_pose_prior_chart")
POINTS_EXPORTS = ("vgicp_points_resident",)
MAP_GATED_EXPORTS = ("vgicp_map_insert_resident_gated", "vgicp_map_insert_resident_gated_async", "vgicp_map_gated_totals")
MAP_CARVE_EXPORTS = ("vgicp_map_carve_resident", "vgicp_map_carve_resident_async", "vgicp_map_carve_totals")
MAP_RAYS_EXPORTS = ("vgicp_rays_resident",)
SEARCH_REPORT_EXPORTS = ("vgicp_prepare_search_report",)   # a test hook
MAP_LEVELS_EXPORTS = ("vgicp_map_levels_build", "vgicp_map_level_size", "vgicp_map_level_export", "vgicp_align_resident_levels")
MAP_LOCATE_EXPORTS = ("vgicp_locate_resident",)
MAP_SUBMAP_EXPORTS = ("vgicp_scan_from_map", "vgicp_scan_from_map_keys")
MAP_CHECKPOINT_EXPORTS = ("vgicp_map_checkpoint_size", "vgicp_map_checkpoint", "vgicp_map_checkpoint_info", "vgicp_map_restore")
MAP_MERGE_EXPORTS = ("vgicp_map_merge",)
SIDE_EXPORTS = {"prior": PRIOR_EXPORTS, "points": POINTS_EXPORTS, "map_gated": MAP_GATED_EXPORTS,
                "map_carve": MAP_CARVE_EXPORTS, "map_rays": MAP_RAYS_EXPORTS, "search_report": SEARCH_REPORT_EXPORTS,
                "map_levels": MAP_LEVELS_EXPORTS, "map_locate": MAP_LOCATE_EXPORTS, "map_submap": MAP_SUBMAP_EXPORTS,
                "map_checkpoint": MAP_CHECKPOINT_EXPORTS, "map_merge": MAP_MERGE_EXPORTS}


def side_lib_path(name: str) -> str:
    return os.path.join(os.path.dirname(LIB_PATH), f"libvgicp_hip_{name}.so")


POINT_QUANTILES_MAX = 16
POINT_MATCHED, POINT_NEGATIVE, POINT_NOT_FINITE = 1, 2, 4
CARVE_MAX_STEPS = 4096
RAYS_MAX_POSES = 64
RAY_NO_RAY, RAY_OPEN, RAY_OWN, RAY_BEHIND, RAY_CONFIRMED, RAY_BLOCKED, RAY_NEAR = range(7)
RAY_CLASS_NAMES = ("no_ray", "open", "own", "behind", "confirmed", "blocked", "near")
LEVELS_MAX = 4
LEVEL_STAGES_MAX = 8
LOCATE_MAX_POSES = 64
LOCATE_MAX_HALF_WIDTH = 32
LOCATE_MAX_CELLS = 4096
# the fourteen paths of the neighbour search, in the order of the struct's fields (and of the kernel's bits)
SEARCH_PATHS = ("home", "crowded", "no_own_cell", "window_is_k", "whole_scan", "clipped", "open2", "open1", "leaf",
                "finest", "compacted", "spilled", "waited", "reranked")


class VgicpError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"vgicp status {code}: {message}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("max_iteration", C.c_int32), ("chunk_iterations", C.c_int32),
                ("translation_sq_threshold", C.c_double), ("cosine_threshold", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class FrameStats(C.Structure):
    _fields_ = [("kernel_launches", C.c_uint64), ("copies", C.c_uint64), ("host_syncs", C.c_uint64),
                ("prepare_us", C.c_double), ("align_us", C.c_double), ("insert_us", C.c_double),
                ("prepare_head_us", C.c_double)]


OPTION_STAGE_EVENTS = 1
OPTION_UPLOAD_STAGE_KB = 2   # scans up to this many KiB are staged through page-locked memory of the context; 0 = in place (vgicp_hip.h)
OPTION_REFERENCE_ORDER = 3   # != 0: scan preparations emit the kept points in the reference's unordered_map order (vgicp_hip.h)
OPTION_MAP_RAW_POINTS = 4    # != 0: the map keeps every voxel's raw points on the device (vgicp_hip_map_points.h)
# robust rounds (vgicp_hip_robust.h): three options, no entry point of their own
OPTION_ROBUST_KERNEL = 5        # ROBUST_NONE (default), ROBUST_HUBER, ROBUST_CAUCHY
OPTION_ROBUST_SCALE_MICRO = 6   # c = value / 1e6, value >= 1; default 1 000 000
OPTION_GATE_MICRO = 7           # gate on d^2 = value / 1e6; 0 = no gate (default)
ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY = 0, 1, 2
ROBUST_EXPORTS = ()
ROBUST_KERNELS = {"none": ROBUST_NONE, "huber": ROBUST_HUBER, "cauchy": ROBUST_CAUCHY}
COUNTER_UPLOAD_SLOW = 6


class SearchReport(C.Structure):
    """vgicp_search_report (vgicp_hip_search_report.h), 96 bytes."""
    _fields_ = [(name, C.c_uint32) for name in
                ("kept", "n_heavy", "n_light", "cells", "spilled_or_swept", "batches_total", "batches_max", "cells_total",
                 "cells_max", "above_voxel") + SEARCH_PATHS]

    def paths(self) -> dict:
        return {name: int(getattr(self, name)) for name in SEARCH_PATHS}

    def line(self) -> str:
        """One line for a log: the start lists, then every path with the queries that took it."""
        return (f"kept {self.kept} heavy {self.n_heavy} light {self.n_light} cells {self.cells} | "
                + " ".join(f"{k} {v}" for k, v in self.paths().items()))


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("world_size", C.c_int32),
                ("launches", C.c_int32), ("seconds", C.c_double), ("device_seconds", C.c_double),
                ("corr_count", C.POINTER(C.c_uint64)), ("normal_eq", C.POINTER(C.c_double)),
                ("kernel_ms", C.POINTER(C.c_float))]


class BatchStats(C.Structure):
    _fields_ = [("hypotheses_per_launch", C.c_int32), ("launches", C.c_int32), ("seconds", C.c_double),
                ("device_seconds", C.c_double),
                ("status", C.POINTER(C.c_int32)), ("iterations", C.POINTER(C.c_int32)),
                ("converged", C.POINTER(C.c_int32)), ("corr_count", C.POINTER(C.c_uint64)),
                ("normal_eq", C.POINTER(C.c_double))]


class Evaluation(C.Structure):
    """vgicp_evaluation (vgicp_hip_evaluate.h), 248 bytes."""
    _fields_ = [("points", C.c_uint64), ("correspondences", C.c_uint64), ("cost", C.c_double),
                ("sq_error", C.c_double), ("normal_eq", C.c_double * 27)]


class EvalStats(C.Structure):
    _fields_ = [("launches", C.c_int32), ("poses_per_launch", C.c_int32), ("seconds", C.c_double),
                ("device_seconds", C.c_double)]


class PointSummary(C.Structure):
    """vgicp_point_summary (vgicp_hip_points.h), 168 bytes."""
    _fields_ = [("points", C.c_uint64), ("matched", C.c_uint64), ("counted", C.c_uint64), ("negative", C.c_uint64),
                ("not_finite", C.c_uint64), ("quantile", C.c_double * POINT_QUANTILES_MAX)]


class PointStats(C.Structure):
    _fields_ = [("launches", C.c_int32), ("reserved", C.c_int32), ("seconds", C.c_double),
                ("device_seconds", C.c_double)]


class GatedInsertStats(C.Structure):
    """vgicp_gated_insert_stats (vgicp_hip_map_gated.h), 64 bytes."""
    _fields_ = [("points", C.c_uint64), ("matched", C.c_uint64), ("refused", C.c_uint64), ("not_finite", C.c_uint64),
                ("new_voxels", C.c_uint64), ("launches", C.c_int32), ("reserved", C.c_int32), ("seconds", C.c_double),
                ("device_seconds", C.c_double)]


class CarveParams(C.Structure):
    """vgicp_carve_params (vgicp_hip_map_carve.h), 48 bytes."""
    _fields_ = [("origin", C.c_double * 3), ("margin", C.c_double), ("max_range", C.c_double),
                ("min_hits", C.c_uint32), ("stride", C.c_uint32)]


class CarveStats(C.Structure):
    """vgicp_carve_stats (vgicp_hip_map_carve.h), 64 bytes."""
    _fields_ = [("rays", C.c_uint64), ("visits", C.c_uint64), ("touched", C.c_uint64), ("shielded", C.c_uint64),
                ("removed", C.c_uint64), ("launches", C.c_int32), ("reserved", C.c_int32), ("seconds", C.c_double),
                ("device_seconds", C.c_double)]


def carve_params(margin: float = 0.0, max_range: float = 80.0, min_hits: int = 1, stride: int = 1,
                 origin=(0.0, 0.0, 0.0)) -> CarveParams:
    return CarveParams((C.c_double * 3)(*[float(v) for v in origin]), float(margin), float(max_range), int(min_hits),
                       int(stride))


class LevelsStats(C.Structure):
    """vgicp_levels_stats (vgicp_hip_map_levels.h), 104 bytes."""
    _fields_ = [("voxels", C.c_uint64 * (LEVELS_MAX + 1)), ("slots", C.c_uint64 * (LEVELS_MAX + 1)), ("levels", C.c_int32),
                ("launches", C.c_int32), ("seconds", C.c_double), ("device_seconds", C.c_double)]


@dataclass
class LevelsBuild:
    """What Context.map_levels_build returns: voxels and slots per level ([0]: the map), and how the call ran."""
    voxels: list
    slots: list
    levels: int
    launches: int
    seconds: float
    device_seconds: float


class LocateParams(C.Structure):
    """vgicp_locate_params (vgicp_hip_map_locate.h), 20 bytes."""
    _fields_ = [("level", C.c_int32), ("window", C.c_int32 * 3), ("stride", C.c_uint32)]


class LocateBest(C.Structure):
    """vgicp_locate_best (vgicp_hip_map_locate.h), 160 bytes."""
    _fields_ = [("hits", C.c_uint32), ("cell", C.c_uint32), ("offset", C.c_int32 * 3), ("points", C.c_uint32),
                ("skipped", C.c_uint32), ("reserved", C.c_uint32), ("pose", C.c_double * 16)]


class LocateStats(C.Structure):
    """vgicp_locate_stats (vgicp_hip_map_locate.h), 24 bytes."""
    _fields_ = [("cells", C.c_int32), ("launches", C.c_int32), ("seconds", C.c_double), ("device_seconds", C.c_double)]


@dataclass
class LocateResult:
    """What Context.locate_resident returns.  best: one dict per pose (hits, cell, offset: a tuple of 3, points, skipped,
    pose: 4x4, the input pose moved by offset * the level's voxel size).  hits: uint32 (k, cells), or None."""
    best: list
    hits: Optional[np.ndarray]
    cells: int
    launches: int
    seconds: float
    device_seconds: float


class SubmapParams(C.Structure):
    """vgicp_submap_params (vgicp_hip_map_submap.h), 176 bytes."""
    _fields_ = [("center", C.c_double * 3), ("radius", C.c_double), ("frame", C.c_double * 16), ("min_count", C.c_uint64),
                ("level", C.c_int32), ("reserved", C.c_int32)]


class SubmapStats(C.Structure):
    """vgicp_submap_stats (vgicp_hip_map_submap.h), 56 bytes."""
    _fields_ = [("voxels", C.c_uint64), ("points", C.c_uint64), ("too_far", C.c_uint64), ("too_few", C.c_uint64),
                ("launches", C.c_int32), ("reserved", C.c_int32), ("seconds", C.c_double), ("device_seconds", C.c_double)]


@dataclass
class SubmapResult:
    """What Context.scan_from_map returns: the counts of vgicp_submap_stats and how the call ran.  points is the size of
    the resident scan now; 0 means that there is none."""
    voxels: int
    points: int
    too_far: int
    too_few: int
    launches: int
    seconds: float
    device_seconds: float


class MergeParams(C.Structure):
    """vgicp_merge_params (vgicp_hip_map_merge.h), 184 bytes."""
    _fields_ = [("center", C.c_double * 3), ("radius", C.c_double), ("frame", C.c_double * 16), ("min_count", C.c_uint64),
                ("max_count", C.c_uint64), ("reserved", C.c_uint64)]


class MergeStats(C.Structure):
    """vgicp_merge_stats (vgicp_hip_map_merge.h), 88 bytes."""
    _fields_ = [("voxels", C.c_uint64), ("selected", C.c_uint64), ("too_far", C.c_uint64), ("too_few", C.c_uint64),
                ("created", C.c_uint64), ("updated", C.c_uint64), ("frozen", C.c_uint64), ("points", C.c_uint64),
                ("launches", C.c_int32), ("reserved", C.c_int32), ("seconds", C.c_double), ("device_seconds", C.c_double)]


@dataclass
class MergeResult:
    """What Context.map_merge returns: the counts of vgicp_merge_stats and how the call ran."""
    voxels: int
    selected: int
    too_far: int
    too_few: int
    created: int
    updated: int
    frozen: int
    points: int
    launches: int
    seconds: float
    device_seconds: float


CHECKPOINT_FORMAT, CHECKPOINT_HEADER_BYTES, CHECKPOINT_RAW_POINTS, CHECKPOINT_RULES = 1, 128, 1, 14


class CheckpointInfo(C.Structure):
    """vgicp_checkpoint_info (vgicp_hip_map_checkpoint.h), 80 bytes."""
    _fields_ = [("format", C.c_uint32), ("header_bytes", C.c_uint32), ("total_bytes", C.c_uint64), ("voxel_size", C.c_double),
                ("slots", C.c_uint64), ("voxels", C.c_uint64), ("tombstones", C.c_uint64), ("raw_points", C.c_uint64),
                ("flags", C.c_uint32), ("record_bytes", C.c_uint32), ("checksum", C.c_uint64), ("rule", C.c_int32),
                ("reserved", C.c_int32)]


class CheckpointStats(C.Structure):
    """vgicp_checkpoint_stats (vgicp_hip_map_checkpoint.h), 56 bytes."""
    _fields_ = [("bytes", C.c_uint64), ("voxels", C.c_uint64), ("tombstones", C.c_uint64), ("raw_points", C.c_uint64),
                ("launches", C.c_int32), ("reserved", C.c_int32), ("seconds", C.c_double), ("device_seconds", C.c_double)]


@dataclass
class CheckpointResult:
    """What Context.map_restore returns (and Context.last_checkpoint holds): vgicp_checkpoint_stats."""
    bytes: int
    voxels: int
    tombstones: int
    raw_points: int
    launches: int
    seconds: float
    device_seconds: float


def _blob_bytes(blob) -> np.ndarray:
    """A blob as a contiguous uint8 array; of a file's content (a shim file: the blob, then a trailer) the blob alone,
    by the header's total_bytes."""
    b = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    if b.size >= CHECKPOINT_HEADER_BYTES and bytes(b[:8]) == b"VGICPMAP":
        total = int(b[16:24].view("<u8")[0])
        if CHECKPOINT_HEADER_BYTES <= total < b.size and bytes(b[total:total + 8]) == b"VGICPTRJ":
            b = b[:total]
    return np.ascontiguousarray(b)


def map_checkpoint_info(blob) -> dict:
    """vgicp_map_checkpoint_info (host only): the header's fields and `rule`, 0 when the blob passes the check, else the
    number of the first rule it fails, with `message` naming it."""
    lib = load_library()
    b = _blob_bytes(blob)
    info = CheckpointInfo()
    rc = lib.vgicp_map_checkpoint_info(b.ctypes.data_as(C.c_void_p), b.size, C.byref(info))
    out = {name: getattr(info, name) for name, _ in CheckpointInfo._fields_ if name != "reserved"}
    out["message"] = "" if rc == OK else lib.vgicp_last_error(None).decode()
    return out


class RayParams(C.Structure):
    """vgicp_ray_params (vgicp_hip_map_rays.h), 56 bytes."""
    _fields_ = [("origin", C.c_double * 3), ("margin", C.c_double), ("beyond", C.c_double), ("max_range", C.c_double),
                ("stride", C.c_uint32), ("reserved", C.c_uint32)]


class RayOutputs(C.Structure):
    """vgicp_ray_outputs (vgicp_hip_map_rays.h), 32 bytes: each plane optional."""
    _fields_ = [("status", C.POINTER(C.c_uint8)), ("range", C.POINTER(C.c_double)), ("hit_key", C.POINTER(C.c_int32)),
                ("steps", C.POINTER(C.c_uint32))]


class RayCounts(C.Structure):
    """vgicp_ray_counts (vgicp_hip_map_rays.h), 80 bytes."""
    _fields_ = [("rays", C.c_uint64), ("visits", C.c_uint64), ("by_class", C.c_uint64 * 8)]


class RayStats(C.Structure):
    """vgicp_ray_stats (vgicp_hip_map_rays.h), 24 bytes."""
    _fields_ = [("launches", C.c_int32), ("groups", C.c_int32), ("seconds", C.c_double), ("device_seconds", C.c_double)]


def ray_params(margin: float = 0.0, beyond: float = 0.0, max_range: float = 80.0, stride: int = 1,
               origin=(0.0, 0.0, 0.0)) -> RayParams:
    return RayParams((C.c_double * 3)(*[float(v) for v in origin]), float(margin), float(beyond), float(max_range),
                     int(stride), 0)


@dataclass
class RayReport:
    """What Context.rays_resident returns.  counts: one dict per pose (rays, visits, by_class: a list of 8).  The planes
    (a single pose with per_point=True, else None): status uint8 (n), range float64 (n; NaN with no hit), hit_key int32
    (n, 3; INT32_MIN with no hit), steps uint32 (n)."""
    counts: list
    status: Optional[np.ndarray]
    range: Optional[np.ndarray]
    hit_key: Optional[np.ndarray]
    steps: Optional[np.ndarray]
    launches: int
    groups: int
    seconds: float
    device_seconds: float


# every entry point's argument types, the module's own and the side libraries'; each returns int but those of RESTYPES
vp, dp, ip, sz = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_size_t
PROTOTYPES = {
    "vgicp_abi_version": [],
    "vgicp_create": [C.c_int, C.POINTER(vp)],
    "vgicp_create_multi": [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)],
    "vgicp_destroy": [vp],
    "vgicp_last_error": [vp],
    "vgicp_device_info": [vp, C.c_char_p, sz, ip, C.POINTER(C.c_uint64)],
    "vgicp_get_counter": [vp, C.c_int, C.POINTER(C.c_uint64)],
    "vgicp_map_reset": [vp, C.c_double, sz],
    "vgicp_map_upsert": [vp, sz, ip, dp, dp],
    "vgicp_map_erase": [vp, sz, ip],
    "vgicp_map_size": [vp, C.POINTER(sz), C.POINTER(sz)],
    "vgicp_map_insert_scan": [vp, sz, dp, dp, dp, sz, C.POINTER(sz)],
    "vgicp_map_insert_resident": [vp, dp, sz, C.POINTER(sz)],
    "vgicp_map_evict": [vp, dp, C.c_double, C.POINTER(sz)],
    "vgicp_map_export": [vp, sz, ip, dp, dp, C.POINTER(C.c_uint64), C.POINTER(sz)],
    "vgicp_align": [vp, sz, dp, dp, dp, C.POINTER(Params), dp, C.POINTER(Stats)],
    "vgicp_scan_upload": [vp, sz, dp, dp],
    "vgicp_align_resident": [vp, dp, C.POINTER(Params), dp, C.POINTER(Stats)],
    "vgicp_accumulate": [vp, sz, dp, dp, dp, dp, dp, C.POINTER(C.c_uint64)],
    "vgicp_solve_step": [vp, dp, dp, C.c_double, C.c_double, C.c_uint32, dp, dp, ip, ip],
    "vgicp_match": [vp, sz, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_uint64), C.POINTER(sz)],
    "vgicp_voxel_index": [vp, sz, dp, ip],
    "vgicp_scan_prepare": [vp, sz, dp, dp, sz, dp, dp, C.c_double, C.c_int, C.POINTER(sz), C.POINTER(C.c_int64)],
    "vgicp_scan_download": [vp, sz, dp, dp, C.POINTER(sz)],
    "vgicp_scan_prepare_async": [vp, sz, dp, dp, sz, dp, dp, C.c_double, C.c_int],
    "vgicp_sweep_stage": [vp, sz, dp, dp, C.POINTER(C.c_uint64)],
    "vgicp_sweep_stage_cloud2": [vp, sz, vp, sz, sz, sz, sz, sz, C.POINTER(C.c_uint64)],
    "vgicp_sweep_unstage": [vp, C.c_uint64],
    "vgicp_scan_fetch_begin": [vp, C.POINTER(sz)],
    "vgicp_scan_fetch_end": [vp, sz, dp, dp, C.POINTER(sz)],
    "vgicp_scan_fetch_sums": [vp, C.POINTER(C.c_uint64)],
    "vgicp_peer_status": [vp],
    "vgicp_scan_prepare_staged_async": [vp, C.c_uint64, sz, dp, dp, C.c_double, C.c_int],
    "vgicp_scan_info": [vp, C.POINTER(sz), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)],
    "vgicp_map_insert_resident_async": [vp, dp, sz],
    "vgicp_get_frame_stats": [vp, C.POINTER(FrameStats), C.c_int],
    "vgicp_set_option": [vp, C.c_int, C.c_int],
    "vgicp_host_register": [vp, vp, sz],
    "vgicp_host_unregister": [vp, vp],
    "vgicp_deskew": [vp, sz, dp, dp, sz, dp, C.POINTER(C.c_int64)],
    "vgicp_preprocess": [vp, sz, dp, C.c_double, C.c_int, sz, dp, dp, C.POINTER(C.c_uint64), C.POINTER(sz)],
    "vgicp_comm_unique_id": [vp, vp],
    "vgicp_comm_init": [vp, C.c_int, C.c_int, vp],
    "vgicp_comm_destroy": [vp],
    "vgicp_peer_export": [vp, vp],
    "vgicp_peer_connect": [vp, C.c_int, C.c_int, vp],
    "vgicp_peer_disconnect": [vp],
    "vgicp_map_points_size": [vp, C.POINTER(sz), C.POINTER(sz)],
    "vgicp_map_points_export": [vp, sz, ip, dp, C.POINTER(sz)],
    "vgicp_align_resident_batch": [vp, sz, dp, C.POINTER(Params), dp, C.POINTER(BatchStats)],
    "vgicp_align_batch_width": [vp, C.POINTER(sz)],
    "vgicp_evaluate_resident": [vp, sz, dp, C.POINTER(Evaluation), C.POINTER(EvalStats)],
    "vgicp_set_pose_prior": [vp, dp, dp],
    "vgicp_pose_prior_chart": [dp, dp, dp, dp],
    "vgicp_points_resident": [vp, dp, sz, dp, dp, dp, C.POINTER(C.c_uint8), sz, dp, C.POINTER(PointSummary),
                             C.POINTER(PointStats)],
    "vgicp_map_insert_resident_gated": [vp, dp, sz, C.c_double, sz, C.POINTER(C.c_uint8), C.POINTER(GatedInsertStats)],
    "vgicp_map_insert_resident_gated_async": [vp, dp, sz, C.c_double],
    "vgicp_map_gated_totals": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "vgicp_map_carve_resident": [vp, dp, C.POINTER(CarveParams), sz, ip, C.POINTER(sz), C.POINTER(CarveStats)],
    "vgicp_map_carve_resident_async": [vp, dp, C.POINTER(CarveParams)],
    "vgicp_map_carve_totals": [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "vgicp_rays_resident": [vp, dp, sz, C.POINTER(RayParams), C.POINTER(RayOutputs), C.POINTER(RayCounts),
                           C.POINTER(RayStats)],
    "vgicp_map_levels_build": [vp, C.c_int, C.POINTER(LevelsStats)],
    "vgicp_map_level_size": [vp, C.c_int, C.POINTER(sz), C.POINTER(sz), dp],
    "vgicp_map_level_export": [vp, C.c_int, sz, ip, dp, dp, C.POINTER(C.c_uint64), C.POINTER(sz)],
    "vgicp_align_resident_levels": [vp, dp, sz, ip, C.POINTER(Params), dp, C.POINTER(Stats)],
    "vgicp_locate_resident": [vp, dp, sz, C.POINTER(LocateParams), C.POINTER(LocateBest), C.POINTER(C.c_uint32),
                             C.POINTER(LocateStats)],
    "vgicp_scan_from_map": [vp, vp, C.POINTER(SubmapParams), C.POINTER(SubmapStats)],
    "vgicp_scan_from_map_keys": [vp, sz, ip, C.POINTER(C.c_uint64), C.POINTER(sz)],
    "vgicp_map_merge": [vp, vp, C.POINTER(MergeParams), C.POINTER(MergeStats)],
    "vgicp_prepare_search_report": [vp, C.POINTER(SearchReport)],
    "vgicp_map_checkpoint_size": [vp, C.POINTER(sz)],
    "vgicp_map_checkpoint": [vp, sz, vp, C.POINTER(sz), C.POINTER(CheckpointStats)],
    "vgicp_map_checkpoint_info": [vp, sz, C.POINTER(CheckpointInfo)],
    "vgicp_map_restore": [vp, vp, sz, C.POINTER(CheckpointStats)],
}
RESTYPES = {"vgicp_last_error": C.c_char_p, "vgicp_peer_status": C.c_char_p}
del vp, dp, ip, sz

_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    """dlopen libvgicp_hip.so and declare its prototypes. Raises if the module is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP module first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C eskf_lio_amd/csrc). "
            "There is no CPU fallback for this path.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)

    def declare(handle, names):   # ... and every name is reached through the one object
        for name in names:
            fn = getattr(handle, name)
            fn.argtypes, fn.restype = PROTOTYPES[name], RESTYPES.get(name, C.c_int)
            setattr(lib, name, fn)

    declare(lib, EXPORTS + MAP_POINTS_EXPORTS + BATCH_EXPORTS + EVALUATE_EXPORTS)
    # the side libraries that were built beside the module (a module of an earlier commit, loaded through VGICP_LIB_PATH
    # for a comparison, has fewer)
    for side, names in SIDE_EXPORTS.items():
        if os.path.exists(side_lib_path(side)):
            declare(C.CDLL(side_lib_path(side), mode=C.RTLD_GLOBAL), names)
    _lib = lib
    return lib


def _f64(a, shape_tail) -> np.ndarray:
    out = np.ascontiguousarray(a, dtype=np.float64)
    if out.size and (out.ndim != 2 or out.shape[1] != shape_tail):
        out = out.reshape(-1, shape_tail)
    return out


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def pose_to_abi(T: np.ndarray) -> np.ndarray:
    """4x4 (row, col) numpy pose -> 16 doubles column-major."""
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).T).reshape(16)


def pose_from_abi(v: np.ndarray) -> np.ndarray:
    return np.asarray(v, dtype=np.float64).reshape(4, 4).T.copy()


class BatchResult(list):
    """What align_resident_batch returns: one AlignResult per guess, and how the batch ran."""

    def __init__(self, hypotheses_per_launch: int = 1, launches: int = 0, seconds: float = 0.0,
                 device_seconds: float = 0.0):
        super().__init__()
        self.hypotheses_per_launch = hypotheses_per_launch
        self.launches = launches
        self.seconds = seconds
        self.device_seconds = device_seconds


class EvaluationList(list):
    """What evaluate_resident returns: one PoseEvaluation per pose, and how the call ran."""

    def __init__(self, launches: int = 0, poses_per_launch: int = 0, seconds: float = 0.0, device_seconds: float = 0.0):
        super().__init__()
        self.launches = launches
        self.poses_per_launch = poses_per_launch
        self.seconds = seconds
        self.device_seconds = device_seconds


@dataclass
class PoseEvaluation:
    """One vgicp_evaluation, with the figures an Open3D-style RegistrationResult derives from it."""
    points: int
    correspondences: int
    cost: float          # sum of e^T (R C R^T + C_voxel)^-1 e over the correspondences
    sq_error: float      # sum of |e|^2 over the correspondences
    normal_eq: np.ndarray  # 27, packed as a row of AlignResult.normal_eq

    @property
    def fitness(self) -> float:
        return self.correspondences / self.points if self.points else 0.0

    @property
    def inlier_rmse(self) -> float:
        return float(np.sqrt(self.sq_error / self.correspondences)) if self.correspondences else 0.0

    @property
    def JTJ(self) -> np.ndarray:
        """6 x 6: the information matrix of the pose."""
        return expand_normal_eq(self.normal_eq)[0][0]

    @property
    def JTr(self) -> np.ndarray:
        return expand_normal_eq(self.normal_eq)[1][0]


@dataclass
class PointReport:
    """What points_resident returns: the per-point arrays that were asked for (else None), the counts, the quantiles in
    the order they were asked, and how the call ran."""
    points: int
    matched: int
    counted: int
    negative: int
    not_finite: int
    quantiles: np.ndarray              # one order statistic of d^2 per requested q
    d2: Optional[np.ndarray] = None    # raw e^T W e; +inf where the point has no voxel
    sq_error: Optional[np.ndarray] = None
    weight: Optional[np.ndarray] = None
    status: Optional[np.ndarray] = None  # uint8: POINT_MATCHED | POINT_NEGATIVE | POINT_NOT_FINITE
    launches: int = 0
    seconds: float = 0.0
    device_seconds: float = 0.0


@dataclass
class AlignResult:
    pose: np.ndarray  # 4x4
    iterations: int
    converged: bool
    world_size: int
    launches: int
    seconds: float
    device_seconds: float
    corr_count: np.ndarray  # per executed iteration
    normal_eq: np.ndarray  # iterations x 27
    kernel_ms: Optional[np.ndarray] = None
    status: int = OK
    message: str = ""
    _expanded: Optional[tuple] = field(default=None, repr=False)

    def _expand(self):
        if self._expanded is None:   # unpacked on first use: diagnostics, not part of an align
            self._expanded = expand_normal_eq(self.normal_eq)
        return self._expanded

    @property
    def JTJ(self) -> np.ndarray:
        """iterations x 6 x 6 (mirrored from the packed lower triangle)."""
        return self._expand()[0]

    @property
    def JTr(self) -> np.ndarray:
        """iterations x 6."""
        return self._expand()[1]


def expand_normal_eq(rows: np.ndarray):
    """iterations x 27 packed rows -> (iterations x 6 x 6 symmetric JTJ, iterations x 6 JTr)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 27)
    JTJ = np.zeros((rows.shape[0], 6, 6))
    k = 0
    for r in range(6):
        for c in range(r + 1):
            JTJ[:, r, c] = rows[:, k]
            JTJ[:, c, r] = rows[:, k]
            k += 1
    return JTJ, rows[:, 21:27].copy()


class Context:
    """One vgicp_ctx: bound to one HIP device, or (a list of ordinals) driving several from this one thread."""

    def __init__(self, device_id=0):
        """device_id: one ordinal, or a sequence of ordinals for an in-process multi-device context
        (vgicp_create_multi; an ordinal may repeat: those sub-contexts share the device's compute units)."""
        self._lib = load_library()
        self._h = C.c_void_p()
        if isinstance(device_id, (list, tuple)):
            ids = (C.c_int * len(device_id))(*[int(d) for d in device_id])
            rc = self._lib.vgicp_create_multi(ids, len(device_id), C.byref(self._h))
        else:
            rc = self._lib.vgicp_create(int(device_id), C.byref(self._h))
        if rc != OK:
            msg = self._lib.vgicp_last_error(None).decode()
            self._h = C.c_void_p()
            raise VgicpError(rc, msg)

    # -- lifetime --
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.vgicp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, allow=()):
        if rc != OK and rc not in allow:
            raise VgicpError(rc, self._lib.vgicp_last_error(self._h).decode())
        return rc

    def last_error(self) -> str:
        return self._lib.vgicp_last_error(self._h).decode()

    def device_info(self):
        name = C.create_string_buffer(64)
        cu = C.c_int32()
        hbm = C.c_uint64()
        self._check(self._lib.vgicp_device_info(self._h, name, 64, C.byref(cu), C.byref(hbm)))
        return name.value.decode(), cu.value, hbm.value

    def counter(self, which: int) -> int:
        """vgicp_get_counter: 0 persistent launches, 1 persistent fallbacks, 2 upload bytes, 3 upload ns,
        4 indefinite covariances of the last scan preparation."""
        v = C.c_uint64(0)
        self._check(self._lib.vgicp_get_counter(self._h, int(which), C.byref(v)))
        return int(v.value)

    # -- map mirror --
    def map_reset(self, voxel_size: float, capacity_hint: int = 0):
        self._check(self._lib.vgicp_map_reset(self._h, float(voxel_size), int(capacity_hint)))

    def map_upsert(self, keys, means, covs):
        keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
        means = _f64(means, 3)
        covs = _f64(covs, 9)
        n = keys.shape[0]
        if means.shape[0] != n or covs.shape[0] != n:
            raise ValueError("keys / means / covs disagree in length")
        self._check(self._lib.vgicp_map_upsert(self._h, n, keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                               _dp(means), _dp(covs)))

    def map_erase(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
        self._check(self._lib.vgicp_map_erase(self._h, keys.shape[0],
                                              keys.ctypes.data_as(C.POINTER(C.c_int32))))

    def map_size(self):
        v, s = C.c_size_t(), C.c_size_t()
        self._check(self._lib.vgicp_map_size(self._h, C.byref(v), C.byref(s)))
        return v.value, s.value

    def map_insert_scan(self, points, covs, transform, max_points_per_voxel: int) -> int:
        """LocalMap::updateLocalMap's insertion loop on the device; returns the number of new voxels."""
        points, covs = _f64(points, 3), _f64(covs, 9)
        if points.shape[0] != covs.shape[0]:
            raise ValueError("points / covs disagree in length")
        T = pose_to_abi(transform)
        new = C.c_size_t()
        self._check(self._lib.vgicp_map_insert_scan(self._h, points.shape[0], _dp(points), _dp(covs), _dp(T),
                                                    int(max_points_per_voxel), C.byref(new)))
        return new.value

    def map_insert_resident(self, transform, max_points_per_voxel: int) -> int:
        """Insert the scan that is already resident (the one the last align registered)."""
        T = pose_to_abi(transform)
        new = C.c_size_t()
        self._check(self._lib.vgicp_map_insert_resident(self._h, _dp(T), int(max_points_per_voxel), C.byref(new)))
        return new.value

    def map_evict(self, position, distance_threshold: float) -> int:
        pos = np.ascontiguousarray(position, dtype=np.float64).reshape(3)
        removed = C.c_size_t()
        self._check(self._lib.vgicp_map_evict(self._h, _dp(pos), float(distance_threshold), C.byref(removed)))
        return removed.value

    def map_export(self):
        """(keys, means, covs, counts) of every voxel in the mirror, sorted by key."""
        n = self.map_size()[0]
        keys = np.zeros((n, 3), dtype=np.int32)
        means, covs = np.zeros((n, 3)), np.zeros((n, 9))
        counts = np.zeros(n, dtype=np.uint64)
        w = C.c_size_t()
        self._check(self._lib.vgicp_map_export(self._h, n, keys.ctypes.data_as(C.POINTER(C.c_int32)), _dp(means),
                                               _dp(covs), counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(w)))
        assert w.value == n
        order = np.lexsort(keys.T)
        return keys[order], means[order], covs[order], counts[order]

    def map_points_size(self):
        """(raw points the map keeps, entries the device store holds before it grows); VgicpError (NOT_READY) while
        OPTION_MAP_RAW_POINTS is off."""
        p, c = C.c_size_t(), C.c_size_t()
        self._check(self._lib.vgicp_map_points_size(self._h, C.byref(p), C.byref(c)))
        return p.value, c.value

    def map_points_export(self):
        """(keys n x 3 int32, points n x 3) of every raw point the map keeps: a voxel's points contiguous, in insertion
        order; the voxels in the library's (unspecified) order."""
        n = self.map_points_size()[0]
        keys = np.zeros((n, 3), dtype=np.int32)
        pts = np.zeros((n, 3))
        w = C.c_size_t()
        self._check(self._lib.vgicp_map_points_export(self._h, n, keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      _dp(pts), C.byref(w)))
        assert w.value == n, (w.value, n)
        return keys, pts

    # -- registration --
    def scan_upload(self, points, covs):
        points, covs = _f64(points, 3), _f64(covs, 9)
        if points.shape[0] != covs.shape[0]:
            raise ValueError("points / covs disagree in length")
        self._check(self._lib.vgicp_scan_upload(self._h, points.shape[0], _dp(points), _dp(covs)))

    def _run(self, call, max_iteration, translation_sq_threshold, cosine_threshold, chunk, flags,
             allow_degenerate):
        p = Params(int(max_iteration), int(chunk), float(translation_sq_threshold),
                   float(cosine_threshold), int(flags), 0)
        cap = max(int(max_iteration), 1)
        # output buffers are kept per context and reused (a call in a frame loop should not pay for a dozen
        # numpy allocations); the result holds copies of the filled parts
        scratch = getattr(self, "_scratch", None)
        if scratch is None or scratch[0] < cap:
            counts = np.zeros(cap, dtype=np.uint64)
            neq = np.zeros((cap, 27))
            kms = np.zeros(cap, dtype=np.float32)
            st = Stats()
            st.corr_count = counts.ctypes.data_as(C.POINTER(C.c_uint64))
            st.normal_eq = _dp(neq)
            st.kernel_ms = kms.ctypes.data_as(C.POINTER(C.c_float))
            out = np.zeros(16)
            scratch = self._scratch = (cap, counts, neq, kms, st, out, _dp(out))
        _, counts, neq, kms, st, out, out_p = scratch
        rc = call(p, out_p, st)
        allow = (ERR_DEGENERATE,) if allow_degenerate else ()
        self._check(rc, allow)
        it = st.iterations
        return AlignResult(pose=pose_from_abi(out), iterations=it, converged=bool(st.converged),
                           world_size=st.world_size, launches=st.launches, seconds=st.seconds,
                           device_seconds=st.device_seconds, corr_count=counts[:it].copy(),
                           normal_eq=neq[:it].copy(),
                           kernel_ms=kms[:st.launches].copy() if flags & FLAG_PROFILE else None,
                           status=rc, message=self.last_error() if rc else "")

    def align(self, points, covs, guess, max_iteration, translation_sq_threshold, cosine_threshold,
              chunk_iterations: int = 0, flags: int = 0, allow_degenerate: bool = False) -> AlignResult:
        points, covs = _f64(points, 3), _f64(covs, 9)
        if points.shape[0] != covs.shape[0]:
            raise ValueError("points / covs disagree in length")
        g = pose_to_abi(guess)
        return self._run(lambda p, out, st: self._lib.vgicp_align(
            self._h, points.shape[0], _dp(points), _dp(covs), _dp(g), C.byref(p), out, C.byref(st)),
            max_iteration, translation_sq_threshold, cosine_threshold, chunk_iterations, flags,
            allow_degenerate)

    def align_resident(self, guess, max_iteration, translation_sq_threshold, cosine_threshold,
                       chunk_iterations: int = 0, flags: int = 0,
                       allow_degenerate: bool = False) -> AlignResult:
        g = pose_to_abi(guess)
        return self._run(lambda p, out, st: self._lib.vgicp_align_resident(
            self._h, _dp(g), C.byref(p), out, C.byref(st)),
            max_iteration, translation_sq_threshold, cosine_threshold, chunk_iterations, flags,
            allow_degenerate)

    def align_resident_batch(self, guesses, max_iteration, translation_sq_threshold, cosine_threshold,
                             flags: int = 0) -> "BatchResult":
        """vgicp_align_resident_batch (vgicp_hip_batch.h): the resident scan from every guess of `guesses` (k 4x4
        poses).  A list of the AlignResults align_resident would return, one per guess (status / message say when a
        hypothesis is degenerate; nothing is raised for that), with hypotheses_per_launch and launches."""
        gs = [pose_to_abi(g) for g in guesses]
        k = len(gs)
        g = np.ascontiguousarray(np.stack(gs).reshape(k, 16)) if k else np.zeros((0, 16))
        cap = max(int(max_iteration), 0)
        p = Params(int(max_iteration), 0, float(translation_sq_threshold), float(cosine_threshold), int(flags), 0)
        out = np.zeros((max(k, 1), 16))
        status = np.zeros(max(k, 1), dtype=np.int32)
        its = np.zeros(max(k, 1), dtype=np.int32)
        conv = np.zeros(max(k, 1), dtype=np.int32)
        counts = np.zeros((max(k, 1), max(cap, 1)), dtype=np.uint64)
        neq = np.zeros((max(k, 1), max(cap, 1), 27))
        i32p = C.POINTER(C.c_int32)
        st = BatchStats()
        st.status, st.iterations, st.converged = (status.ctypes.data_as(i32p), its.ctypes.data_as(i32p),
                                                  conv.ctypes.data_as(i32p))
        # the ABI's layout is k x max_iteration (x 27): the arrays above have exactly that stride when cap >= 1
        st.corr_count = counts.ctypes.data_as(C.POINTER(C.c_uint64))
        st.normal_eq = _dp(neq)
        self._check(self._lib.vgicp_align_resident_batch(self._h, k, _dp(g), C.byref(p), _dp(out), C.byref(st)))
        res = BatchResult(hypotheses_per_launch=st.hypotheses_per_launch, launches=st.launches, seconds=st.seconds,
                          device_seconds=st.device_seconds)
        for h in range(k):
            it = int(its[h])
            res.append(AlignResult(pose=pose_from_abi(out[h]), iterations=it, converged=bool(conv[h]),
                                   world_size=1, launches=st.launches, seconds=st.seconds,
                                   device_seconds=st.device_seconds, corr_count=counts[h, :it].copy(),
                                   normal_eq=neq[h, :it].copy(), kernel_ms=None, status=int(status[h]),
                                   message="solved pose is not finite" if status[h] else ""))
        return res

    def evaluate_resident(self, poses) -> "EvaluationList":
        """vgicp_evaluate_resident (vgicp_hip_evaluate.h): the resident scan scored at every pose of `poses` (k 4x4
        poses): a list of PoseEvaluation, with launches and poses_per_launch."""
        gs = [pose_to_abi(g) for g in poses]
        k = len(gs)
        g = np.ascontiguousarray(np.stack(gs).reshape(k, 16)) if k else np.zeros((0, 16))
        out = (Evaluation * max(k, 1))()
        st = EvalStats()
        self._check(self._lib.vgicp_evaluate_resident(self._h, k, _dp(g), out, C.byref(st)))
        res = EvaluationList(st.launches, st.poses_per_launch, st.seconds, st.device_seconds)
        for h in range(k):
            res.append(PoseEvaluation(points=int(out[h].points), correspondences=int(out[h].correspondences),
                                      cost=float(out[h].cost), sq_error=float(out[h].sq_error),
                                      normal_eq=np.array(out[h].normal_eq[:], dtype=np.float64)))
        return res

    def points_size(self) -> int:
        """n of the resident scan (a pending preparation is settled): vgicp_scan_download's size query."""
        n = C.c_size_t(0)
        self._check(self._lib.vgicp_scan_download(self._h, 0, None, None, C.byref(n)))
        return int(n.value)

    def points_resident(self, pose, quantiles=(), d2=True, sq_error=True, weight=True, status=True) -> "PointReport":
        """vgicp_points_resident (vgicp_hip_points.h): the resident scan at `pose`, point by point — raw d^2, |e|^2, the
        weight under the context's robust options and the status flags, for the arrays asked — with the counts and the
        order statistics of d^2 at `quantiles` (each in [0, 1], at most 16)."""
        T = pose_to_abi(pose)
        qs = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        summary, st = PointSummary(), PointStats()
        n = self.points_size() if (d2 or sq_error or weight or status) else 0
        a_d2 = np.zeros(n) if d2 else None
        a_sq = np.zeros(n) if sq_error else None
        a_w = np.zeros(n) if weight else None
        a_st = np.zeros(n, dtype=np.uint8) if status else None
        self._check(self._lib.vgicp_points_resident(
            self._h, _dp(T), n, _dp(a_d2) if d2 else None, _dp(a_sq) if sq_error else None, _dp(a_w) if weight else None,
            a_st.ctypes.data_as(C.POINTER(C.c_uint8)) if status else None, qs.size, _dp(qs) if qs.size else None,
            C.byref(summary), C.byref(st)))
        return PointReport(points=int(summary.points), matched=int(summary.matched), counted=int(summary.counted),
                           negative=int(summary.negative), not_finite=int(summary.not_finite),
                           quantiles=np.array(summary.quantile[:qs.size], dtype=np.float64), d2=a_d2, sq_error=a_sq,
                           weight=a_w, status=a_st, launches=st.launches, seconds=st.seconds,
                           device_seconds=st.device_seconds)

    def align_batch_width(self) -> int:
        """vgicp_align_batch_width: hypotheses one launch takes for the scan that is resident now."""
        w = C.c_size_t(0)
        self._check(self._lib.vgicp_align_batch_width(self._h, C.byref(w)))
        return int(w.value)

    # -- hooks --
    def accumulate(self, points, covs, pose):
        points, covs = _f64(points, 3), _f64(covs, 9)
        g = pose_to_abi(pose)
        JTJ, JTr, cnt = np.zeros(36), np.zeros(6), C.c_uint64()
        self._check(self._lib.vgicp_accumulate(self._h, points.shape[0], _dp(points), _dp(covs), _dp(g),
                                               _dp(JTJ), _dp(JTr), C.byref(cnt)))
        return JTJ.reshape(6, 6).T.copy(), JTr, cnt.value

    def solve_step(self, JTJ, JTr, cosine_threshold: float = 0.9999, translation_sq_threshold: float = 1e-6,
                   force_pivoted: bool = False):
        """ldlt().solve(-JTr) + se3ToSE3 + convergenceCheck on the device -> (se3, step 4x4, used_pivoted,
        converged). JTJ: 6x6 (row, col) numpy; only its lower triangle is read."""
        A = np.ascontiguousarray(np.asarray(JTJ, dtype=np.float64).reshape(6, 6).T).reshape(36)
        b = np.ascontiguousarray(JTr, dtype=np.float64).reshape(6)
        se3, step = np.zeros(6), np.zeros(16)
        piv, conv = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.vgicp_solve_step(self._h, _dp(A), _dp(b), float(cosine_threshold),
                                               float(translation_sq_threshold),
                                               SOLVE_FORCE_PIVOTED if force_pivoted else 0, _dp(se3), _dp(step),
                                               C.byref(piv), C.byref(conv)))
        return se3, pose_from_abi(step), bool(piv.value), bool(conv.value)

    def match(self, points, covs):
        points, covs = _f64(points, 3), _f64(covs, 9)
        n = points.shape[0]
        sp, sc, mp, mc = np.zeros((n, 3)), np.zeros((n, 9)), np.zeros((n, 3)), np.zeros((n, 9))
        ix = np.zeros(n, dtype=np.uint64)
        m = C.c_size_t()
        self._check(self._lib.vgicp_match(self._h, n, _dp(points), _dp(covs), _dp(sp), _dp(sc), _dp(mp),
                                          _dp(mc), ix.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(m)))
        k = m.value
        return sp[:k], sc[:k], mp[:k], mc[:k], ix[:k]

    def voxel_index(self, points) -> np.ndarray:
        points = _f64(points, 3)
        keys = np.zeros((points.shape[0], 3), dtype=np.int32)
        self._check(self._lib.vgicp_voxel_index(self._h, points.shape[0], _dp(points),
                                                keys.ctypes.data_as(C.POINTER(C.c_int32))))
        return keys

    def search_report(self, start_lists_only: bool = False) -> "SearchReport":
        """vgicp_prepare_search_report (vgicp_hip_search_report.h): the paths the neighbour search of the last settled
        preparation took, from a context created under VGICP_DEBUG_PREP.  Any other context is refused
        (ERR_BAD_ARGUMENT) unless start_lists_only: then kept, n_heavy and n_light, which every context has, are
        returned and the rest is zero.  ERR_NOT_READY before any preparation has been settled."""
        r = SearchReport()
        rc = self._lib.vgicp_prepare_search_report(self._h, C.byref(r))
        if not (start_lists_only and rc == ERR_BAD_ARGUMENT and "VGICP_DEBUG_PREP" in self.last_error()):
            self._check(rc)
        return r

    def preprocess(self, points, voxel_size: float, knn: int = 30):
        """CloudPreprocessor::voxelDownsampleAndEstimateCovariances (CloudPreprocessor.cpp:76-127) on the
        device -> (kept points m x 3, covariances m x 9 column-major, indices of the kept points)."""
        points = _f64(points, 3)
        n = points.shape[0]
        op, oc = np.zeros((n, 3)), np.zeros((n, 9))
        ix = np.zeros(n, dtype=np.uint64)
        m = C.c_size_t(0)
        self._check(self._lib.vgicp_preprocess(self._h, n, _dp(points), float(voxel_size), int(knn), n, _dp(op),
                                               _dp(oc), ix.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(m)))
        k = m.value
        return op[:k].copy(), oc[:k].copy(), ix[:k].copy()

    def deskew(self, points, point_time, states):
        """CloudPreprocessor::deskew (CloudPreprocessor.cpp:25-74) on the device. states: S x 8 (timestamp,
        position, quaternion x y z w). -> (points, count); count is -1 with the points unchanged where the
        reference would run off its state queue."""
        pts = _f64(points, 3).copy()
        t = np.ascontiguousarray(point_time, dtype=np.float64).reshape(-1)
        st = _f64(states, 8)
        if t.shape[0] != pts.shape[0]:
            raise ValueError("one capture time per point")
        done = C.c_int64(0)
        self._check(self._lib.vgicp_deskew(self._h, pts.shape[0], _dp(pts), _dp(t), st.shape[0], _dp(st),
                                           C.byref(done)))
        return pts, int(done.value)

    def scan_prepare(self, points, point_time=None, states=None, extrinsic=None, voxel_size: float = 0.3,
                     knn: int = 30):
        """CloudPreprocessor::process on the device, the prepared scan stays resident -> (kept, deskewed)."""
        pts = _f64(points, 3)
        n = pts.shape[0]
        st = _f64(states, 8) if states is not None and len(states) else np.zeros((0, 8))
        t = np.ascontiguousarray(point_time, dtype=np.float64).reshape(-1) if point_time is not None else np.zeros(0)
        if st.shape[0] and t.shape[0] != n:
            raise ValueError("one capture time per point")
        ext = pose_to_abi(extrinsic) if extrinsic is not None else None
        kept, moved = C.c_size_t(0), C.c_int64(0)
        self._check(self._lib.vgicp_scan_prepare(self._h, n, _dp(pts), _dp(t) if t.size else None, st.shape[0],
                                                 _dp(st) if st.size else None, _dp(ext) if ext is not None else None,
                                                 float(voxel_size), int(knn), C.byref(kept), C.byref(moved)))
        return kept.value, int(moved.value)

    def scan_prepare_async(self, points, point_time=None, states=None, extrinsic=None, voxel_size: float = 0.3,
                           knn: int = 30):
        """vgicp_scan_prepare_async: the same, only enqueued (nothing waited for, nothing returned)."""
        pts = _f64(points, 3)
        n = pts.shape[0]
        st = _f64(states, 8) if states is not None and len(states) else np.zeros((0, 8))
        t = np.ascontiguousarray(point_time, dtype=np.float64).reshape(-1) if point_time is not None else np.zeros(0)
        if st.shape[0] and t.shape[0] != n:
            raise ValueError("one capture time per point")
        ext = pose_to_abi(extrinsic) if extrinsic is not None else None
        self._check(self._lib.vgicp_scan_prepare_async(self._h, n, _dp(pts), _dp(t) if t.size else None, st.shape[0],
                                                       _dp(st) if st.size else None, _dp(ext) if ext is not None else None,
                                                       float(voxel_size), int(knn)))

    def peer_status(self) -> str:
        """vgicp_peer_status: "" while the kernels' own mailboxes carry the merge between devices, else why not."""
        return self._lib.vgicp_peer_status(self._h).decode()

    def sweep_stage(self, points, point_time=None) -> int:
        """vgicp_sweep_stage: a raw sweep copied into page-locked memory of the context when it arrives -> ticket."""
        pts = _f64(points, 3)
        t = np.ascontiguousarray(point_time, dtype=np.float64).reshape(-1) if point_time is not None else np.zeros(0)
        if t.size and t.shape[0] != pts.shape[0]:
            raise ValueError("one capture time per point")
        ticket = C.c_uint64(0)
        self._check(self._lib.vgicp_sweep_stage(self._h, pts.shape[0], _dp(pts), _dp(t) if t.size else None, C.byref(ticket)))
        return int(ticket.value)

    def scan_fetch(self):
        """vgicp_scan_fetch_begin + _end: the prepared scan of a pending (enqueued) preparation -> (points, covs)."""
        kept = C.c_size_t(0)
        self._check(self._lib.vgicp_scan_fetch_begin(self._h, C.byref(kept)))
        pts, covs = np.zeros((kept.value, 3)), np.zeros((kept.value, 9))
        n = C.c_size_t(0)
        self._check(self._lib.vgicp_scan_fetch_end(self._h, kept.value, _dp(pts) if kept.value else None,
                                                  _dp(covs) if kept.value else None, C.byref(n)))
        assert n.value == kept.value
        return pts, covs

    def scan_fetch_begin(self) -> int:
        """vgicp_scan_fetch_begin alone: the fetch kernel enqueued behind the pending preparation -> the kept count."""
        kept = C.c_size_t(0)
        self._check(self._lib.vgicp_scan_fetch_begin(self._h, C.byref(kept)))
        return kept.value

    def scan_fetch_end(self, capacity: int):
        """vgicp_scan_fetch_end alone, into arrays of `capacity` points -> (points, covs) of the delivered size."""
        cap = int(capacity)
        pts, covs = np.zeros((cap, 3)), np.zeros((cap, 9))
        n = C.c_size_t(0)
        self._check(self._lib.vgicp_scan_fetch_end(self._h, cap, _dp(pts) if cap else None, _dp(covs) if cap else None,
                                                  C.byref(n)))
        return pts[:n.value].copy(), covs[:n.value].copy()

    def scan_fetch_sums(self) -> np.ndarray:
        """vgicp_scan_fetch_sums: the device-made checksums of the last scan_fetch -> uint64[2][2][16] (array, A / B, lane)."""
        out = np.zeros(64, dtype=np.uint64)
        self._check(self._lib.vgicp_scan_fetch_sums(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out.reshape(2, 2, 16)

    def sweep_unstage(self, ticket: int) -> None:
        """vgicp_sweep_unstage: drop a staged sweep that will not be prepared (its slot is free again)."""
        self._check(self._lib.vgicp_sweep_unstage(self._h, C.c_uint64(int(ticket))))

    def sweep_stage_cloud2(self, data, n: int, point_step: int, off_x: int, off_y: int, off_z: int, off_time=None) -> int:
        """vgicp_sweep_stage_cloud2: the payload of a PointCloud2 (bytes / uint8 array, little-endian records) as it
        arrives; the device widens the float32 coordinates -> ticket."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if buf.size < n * point_step:
            raise ValueError("payload shorter than n * point_step")
        ticket = C.c_uint64(0)
        self._check(self._lib.vgicp_sweep_stage_cloud2(self._h, int(n), buf.ctypes.data_as(C.c_void_p), int(point_step), int(off_x),
                                                       int(off_y), int(off_z), (2 ** 64 - 1) if off_time is None else int(off_time),
                                                       C.byref(ticket)))
        return int(ticket.value)

    def scan_prepare_staged_async(self, ticket: int, states=None, extrinsic=None, voxel_size: float = 0.3, knn: int = 30):
        """vgicp_scan_prepare_staged_async: vgicp_scan_prepare_async for a sweep staged by sweep_stage."""
        st = _f64(states, 8) if states is not None and len(states) else np.zeros((0, 8))
        ext = pose_to_abi(extrinsic) if extrinsic is not None else None
        self._check(self._lib.vgicp_scan_prepare_staged_async(self._h, int(ticket), st.shape[0], _dp(st) if st.size else None,
                                                              _dp(ext) if ext is not None else None, float(voxel_size), int(knn)))

    def scan_info(self):
        """(kept points, what the deskew reports, indefinite covariances) of the last preparation."""
        kept, moved, bad = C.c_size_t(0), C.c_int64(0), C.c_uint64(0)
        self._check(self._lib.vgicp_scan_info(self._h, C.byref(kept), C.byref(moved), C.byref(bad)))
        return kept.value, int(moved.value), int(bad.value)

    def map_insert_resident_async(self, transform, max_points_per_voxel: int):
        T = pose_to_abi(transform)
        self._check(self._lib.vgicp_map_insert_resident_async(self._h, _dp(T), int(max_points_per_voxel)))

    def map_insert_resident_gated(self, transform, max_points_per_voxel: int, gate: float, kept: bool = True):
        """vgicp_map_insert_resident_gated (vgicp_hip_map_gated.h): insert the resident scan without the points that are
        matched at `transform` and fail max(d^2, 0) <= gate.  Returns (kept, stats): a uint8 array, 1 kept and 0 refused
        (None unless asked), and the call's GatedInsertStats."""
        T = pose_to_abi(transform)
        st = GatedInsertStats()
        n = self.points_size() if kept else 0
        a_kept = np.zeros(n, dtype=np.uint8) if kept else None
        self._check(self._lib.vgicp_map_insert_resident_gated(
            self._h, _dp(T), int(max_points_per_voxel), float(gate), n,
            a_kept.ctypes.data_as(C.POINTER(C.c_uint8)) if kept else None, C.byref(st)))
        return a_kept, st

    def map_insert_resident_gated_async(self, transform, max_points_per_voxel: int, gate: float):
        T = pose_to_abi(transform)
        self._check(self._lib.vgicp_map_insert_resident_gated_async(self._h, _dp(T), int(max_points_per_voxel),
                                                                    float(gate)))

    def map_gated_totals(self):
        """(points seen, points refused) by this context's gated insertions since the last map_reset."""
        p, r = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.vgicp_map_gated_totals(self._h, C.byref(p), C.byref(r)))
        return int(p.value), int(r.value)

    def map_carve_resident(self, transform, params, keys: bool = True):
        """vgicp_map_carve_resident (vgicp_hip_map_carve.h): remove the voxels the resident scan sees through at
        `transform`.  params: a CarveParams or what carve_params() takes as keywords.  Returns (removed keys as int32
        (m, 3) in unspecified order, or None unless asked; the call's CarveStats)."""
        T = pose_to_abi(transform)
        p = params if isinstance(params, CarveParams) else carve_params(**params)
        st = CarveStats()
        room = self.map_size()[0] if keys else 0
        a_keys = np.zeros((room, 3), dtype=np.int32) if keys else None
        removed = C.c_size_t(0)
        self._check(self._lib.vgicp_map_carve_resident(
            self._h, _dp(T), C.byref(p), room, a_keys.ctypes.data_as(C.POINTER(C.c_int32)) if room else None,
            C.byref(removed), C.byref(st)))
        return (a_keys[:removed.value].copy() if keys else None), st

    def map_carve_resident_async(self, transform, params):
        T = pose_to_abi(transform)
        p = params if isinstance(params, CarveParams) else carve_params(**params)
        self._check(self._lib.vgicp_map_carve_resident_async(self._h, _dp(T), C.byref(p)))

    def map_carve_totals(self):
        """(rays cast, voxels removed) by this context's carving calls since the last map_reset."""
        r, m = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.vgicp_map_carve_totals(self._h, C.byref(r), C.byref(m)))
        return int(r.value), int(m.value)

    # -- the map's coarser levels (vgicp_hip_map_levels.h) --
    def map_levels_build(self, levels: int) -> "LevelsBuild":
        """vgicp_map_levels_build: ask for `levels` levels (0 .. LEVELS_MAX; 0 releases them) and bring them up to date."""
        st = LevelsStats()
        self._check(self._lib.vgicp_map_levels_build(self._h, int(levels), C.byref(st)))
        return LevelsBuild(list(st.voxels), list(st.slots), st.levels, st.launches, st.seconds, st.device_seconds)

    def map_level_size(self, level: int):
        """(voxels, table slots, voxel size) of a level; level 0 is the map."""
        v, s, h = C.c_size_t(), C.c_size_t(), C.c_double()
        self._check(self._lib.vgicp_map_level_size(self._h, int(level), C.byref(v), C.byref(s), C.byref(h)))
        return v.value, s.value, h.value

    def map_level_export(self, level: int):
        """(keys, means, covs, counts) of every voxel of a level, sorted by key as map_export sorts."""
        n = self.map_level_size(level)[0]
        keys = np.zeros((n, 3), dtype=np.int32)
        means, covs = np.zeros((n, 3)), np.zeros((n, 9))
        counts = np.zeros(n, dtype=np.uint64)
        w = C.c_size_t()
        self._check(self._lib.vgicp_map_level_export(self._h, int(level), n, keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     _dp(means), _dp(covs), counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                     C.byref(w)))
        assert w.value == n, (w.value, n)
        order = np.lexsort(keys.T)
        return keys[order], means[order], covs[order], counts[order]

    def align_resident_levels(self, guess, schedule, params, allow_degenerate: bool = False):
        """vgicp_align_resident_levels: the resident scan in stages.  schedule: the level of every stage; params: per
        stage a dict with max_iteration, translation_sq_threshold, cosine_threshold and optionally chunk_iterations and
        flags (or one dict for all stages).  Returns (pose 4x4, [AlignResult per stage])."""
        schedule = [int(l) for l in schedule]
        k = len(schedule)
        per = [params] * k if isinstance(params, dict) else list(params)
        if len(per) != k:
            raise ValueError("schedule / params disagree in length")
        ps = (Params * max(k, 1))(*[Params(int(p["max_iteration"]), int(p.get("chunk_iterations", 0)),
                                           float(p["translation_sq_threshold"]), float(p["cosine_threshold"]),
                                           int(p.get("flags", 0)), 0) for p in per])
        caps = [max(int(p["max_iteration"]), 1) for p in per]
        counts = [np.zeros(c, dtype=np.uint64) for c in caps]
        neqs = [np.zeros((c, 27)) for c in caps]
        kms = [np.zeros(c + 1, dtype=np.float32) for c in caps]
        sts = (Stats * max(k, 1))()
        for i in range(k):
            sts[i].corr_count = counts[i].ctypes.data_as(C.POINTER(C.c_uint64))
            sts[i].normal_eq = _dp(neqs[i])
            sts[i].kernel_ms = kms[i].ctypes.data_as(C.POINTER(C.c_float))
        lv = (C.c_int32 * max(k, 1))(*schedule)
        g = pose_to_abi(guess)
        out = np.zeros(16)
        rc = self._lib.vgicp_align_resident_levels(self._h, _dp(g), k, lv, ps, _dp(out), sts)
        self._check(rc, (ERR_DEGENERATE,) if allow_degenerate else ())
        stages = []
        for i in range(k):
            st, it = sts[i], sts[i].iterations
            stages.append(AlignResult(pose=None, iterations=it, converged=bool(st.converged), world_size=st.world_size,
                                      launches=st.launches, seconds=st.seconds, device_seconds=st.device_seconds,
                                      corr_count=counts[i][:it].copy(), normal_eq=neqs[i][:it].copy(), status=rc,
                                      message=self.last_error() if rc else ""))
        return pose_from_abi(out), stages

    def locate_resident(self, poses, level: int, window, stride: int = 1, planes: bool = True) -> "LocateResult":
        """vgicp_locate_resident (vgicp_hip_map_locate.h): `poses` (one 4x4 pose or k of them) of the resident scan scored
        over the window of whole-voxel shifts (half-widths wx, wy, wz) on a level of the map, read-only.  planes: also
        the k x cells array of hits."""
        ps = np.asarray(poses, dtype=np.float64)
        ps = ps.reshape(1, 4, 4) if ps.ndim == 2 else ps
        k = len(ps)
        g = np.ascontiguousarray(np.stack([pose_to_abi(T) for T in ps]).reshape(k, 16)) if k else np.zeros((0, 16))
        w = [int(v) for v in window]
        p = LocateParams(int(level), (C.c_int32 * 3)(*w), int(stride))
        cells = (2 * w[0] + 1) * (2 * w[1] + 1) * (2 * w[2] + 1)
        room = cells if all(0 <= v <= LOCATE_MAX_HALF_WIDTH for v in w) and cells <= LOCATE_MAX_CELLS else 1
        hits = np.zeros((k, room), dtype=np.uint32) if planes else None
        best = (LocateBest * max(k, 1))()
        st = LocateStats()
        self._check(self._lib.vgicp_locate_resident(self._h, _dp(g), k, C.byref(p), best,
                                                    hits.ctypes.data_as(C.POINTER(C.c_uint32)) if planes else None,
                                                    C.byref(st)))
        out = [dict(hits=int(b.hits), cell=int(b.cell), offset=tuple(int(v) for v in b.offset), points=int(b.points),
                    skipped=int(b.skipped), pose=pose_from_abi(np.array(b.pose))) for b in best[:k]]
        return LocateResult(out, hits, st.cells, st.launches, st.seconds, st.device_seconds)

    # -- submap as scan (vgicp_hip_map_submap.h) --
    def scan_from_map(self, src: "Context", center, radius: float, frame=None, min_count: int = 0,
                      level: int = 0) -> "SubmapResult":
        """vgicp_scan_from_map: this context's resident scan becomes the voxels of `src`'s map (or of its level `level`)
        whose centres lie within `radius` of `center` (the source map's frame; math.inf: all of them) and whose count is
        at least min_count, each moved by `frame` (4x4, default the identity), in ascending slot order.  src may be self."""
        p = SubmapParams((C.c_double * 3)(*[float(v) for v in center]), float(radius),
                         (C.c_double * 16)(*pose_to_abi(np.eye(4) if frame is None else frame)), int(min_count), int(level), 0)
        st = SubmapStats()
        self._check(self._lib.vgicp_scan_from_map(self._h, src._h, C.byref(p), C.byref(st)))
        return SubmapResult(int(st.voxels), int(st.points), int(st.too_far), int(st.too_few), st.launches, st.seconds,
                            st.device_seconds)

    def scan_from_map_keys(self):
        """vgicp_scan_from_map_keys: (keys n x 3 int32, counts n uint64) of the voxels behind the resident scan that
        scan_from_map made, in scan order; VgicpError (NOT_READY) once the scan has been replaced."""
        w = C.c_size_t()
        rc = self._lib.vgicp_scan_from_map_keys(self._h, 0, None, None, C.byref(w))   # size query
        if rc != OK and not (rc == ERR_BAD_ARGUMENT and w.value > 0):
            self._check(rc)
        n = w.value
        keys, counts = np.zeros((n, 3), dtype=np.int32), np.zeros(n, dtype=np.uint64)
        self._check(self._lib.vgicp_scan_from_map_keys(self._h, n, keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(w)))
        assert w.value == n, (w.value, n)
        return keys, counts

    # -- map merge (vgicp_hip_map_merge.h) --
    def map_merge(self, src: "Context", center=None, radius: float = math.inf, frame=None, min_count: int = 0,
                  max_count: int = 0) -> "MergeResult":
        """vgicp_map_merge: the voxels of `src`'s map whose centres lie within `radius` of `center` (the source map's
        frame; default: all of them) and whose count is at least min_count, each moved by `frame` (4x4, source map ->
        this map, default the identity), are folded into this context's map, weighted by their counts, in ascending slot
        order of the source.  A voxel of this map that holds max_count points or more accepts nothing (0: no cap)."""
        p = MergeParams((C.c_double * 3)(*[float(v) for v in ((0.0, 0.0, 0.0) if center is None else center)]), float(radius),
                        (C.c_double * 16)(*pose_to_abi(np.eye(4) if frame is None else frame)), int(min_count), int(max_count), 0)
        st = MergeStats()
        self._check(self._lib.vgicp_map_merge(self._h, src._h, C.byref(p), C.byref(st)))
        return MergeResult(int(st.voxels), int(st.selected), int(st.too_far), int(st.too_few), int(st.created), int(st.updated),
                           int(st.frozen), int(st.points), st.launches, st.seconds, st.device_seconds)

    # -- map checkpoint (vgicp_hip_map_checkpoint.h) --
    def map_checkpoint_size(self) -> int:
        w = C.c_size_t()
        self._check(self._lib.vgicp_map_checkpoint_size(self._h, C.byref(w)))
        return w.value

    def map_checkpoint(self) -> np.ndarray:
        """vgicp_map_checkpoint: the map as one blob (uint8 array), packed on the device; read-only.  The call's stats
        stay in self.last_checkpoint."""
        blob = np.zeros(self.map_checkpoint_size(), dtype=np.uint8)
        w, st = C.c_size_t(), CheckpointStats()
        self._check(self._lib.vgicp_map_checkpoint(self._h, blob.size, blob.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(st)))
        assert w.value == blob.size, (w.value, blob.size)
        self.last_checkpoint = CheckpointResult(int(st.bytes), int(st.voxels), int(st.tombstones), int(st.raw_points),
                                                st.launches, st.seconds, st.device_seconds)
        return blob

    def map_restore(self, blob) -> "CheckpointResult":
        """vgicp_map_restore: this context's map becomes the blob's, slot for slot.  blob: a uint8 array or bytes; the
        content of a file the shim's saveCheckpoint wrote is read by total_bytes, its trailer ignored."""
        b = _blob_bytes(blob)
        st = CheckpointStats()
        self._check(self._lib.vgicp_map_restore(self._h, b.ctypes.data_as(C.c_void_p), b.size, C.byref(st)))
        return CheckpointResult(int(st.bytes), int(st.voxels), int(st.tombstones), int(st.raw_points), st.launches,
                                st.seconds, st.device_seconds)

    def rays_resident(self, poses, params, per_point: bool = True) -> "RayReport":
        """vgicp_rays_resident (vgicp_hip_map_rays.h): the first map voxel on every ray of the resident scan at `poses`
        (one 4x4 pose or k of them), read-only.  params: a RayParams or what ray_params() takes as keywords.  The planes
        come with a single pose and per_point=True."""
        ps = np.asarray(poses, dtype=np.float64)
        ps = ps.reshape(1, 4, 4) if ps.ndim == 2 else ps
        k = len(ps)
        g = np.ascontiguousarray(np.stack([pose_to_abi(T) for T in ps]).reshape(k, 16)) if k else np.zeros((0, 16))
        p = params if isinstance(params, RayParams) else ray_params(**params)
        planes = per_point and k == 1
        n = self.points_size() if planes else 0
        status = np.zeros(n, dtype=np.uint8) if planes else None
        rng = np.zeros(n) if planes else None
        keys = np.zeros((n, 3), dtype=np.int32) if planes else None
        steps = np.zeros(n, dtype=np.uint32) if planes else None
        out = RayOutputs(status.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(rng), keys.ctypes.data_as(C.POINTER(C.c_int32)),
                         steps.ctypes.data_as(C.POINTER(C.c_uint32))) if planes else None
        counts = (RayCounts * max(k, 1))()
        st = RayStats()
        self._check(self._lib.vgicp_rays_resident(self._h, _dp(g), k, C.byref(p), C.byref(out) if planes else None, counts,
                                                  C.byref(st)))
        return RayReport([dict(rays=int(c.rays), visits=int(c.visits), by_class=[int(v) for v in c.by_class]) for c in counts[:k]],
                         status, rng, keys, steps, st.launches, st.groups, st.seconds, st.device_seconds)

    def frame_stats(self, reset: bool = False) -> FrameStats:
        st = FrameStats()
        self._check(self._lib.vgicp_get_frame_stats(self._h, C.byref(st), 1 if reset else 0))
        return st

    def set_option(self, option: int, value: int):
        self._check(self._lib.vgicp_set_option(self._h, int(option), int(value)))

    def set_robust(self, kernel=ROBUST_NONE, scale: float = 1.0, gate: float = 0.0):
        """The robust round of vgicp_hip_robust.h for every later align of this context: kernel (ROBUST_* or "none" /
        "huber" / "cauchy"), its scale c and the gate on d^2 (0 = none), in the library's regularised units (~0.1, not
        ~3).  The ABI takes millionths: returns (kernel, c, gate) as the library will use them.  Nothing is changed when
        a value is refused."""
        kind = ROBUST_KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        scale_micro, gate_micro = int(round(float(scale) * 1e6)), int(round(float(gate) * 1e6))
        if kind not in (ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY) or not 1 <= scale_micro <= 2**31 - 1 or \
                not 0 <= gate_micro <= 2**31 - 1:
            raise ValueError("robust kernel must be none / huber / cauchy, scale in [1e-6, 2147.48], gate in [0, 2147.48]")
        self.set_option(OPTION_ROBUST_KERNEL, kind)
        self.set_option(OPTION_ROBUST_SCALE_MICRO, scale_micro)
        self.set_option(OPTION_GATE_MICRO, gate_micro)
        return kind, scale_micro / 1000000.0, gate_micro / 1000000.0

    def set_pose_prior(self, prior_pose=None, information=None):
        """vgicp_set_pose_prior (vgicp_hip_prior.h): a Gaussian prior on the pose for every later align of this context
        — prior_pose 4x4, information 6x6 in the filter's chart [t - t0; Log(R0^T R)].  None for either, or an all-zero
        information, clears it.  Nothing is changed when a value is refused."""
        if prior_pose is None or information is None:
            self._check(self._lib.vgicp_set_pose_prior(self._h, None, None))
            return
        info = np.ascontiguousarray(np.asarray(information, dtype=np.float64).reshape(6, 6).T).reshape(36)
        self._check(self._lib.vgicp_set_pose_prior(self._h, _dp(pose_to_abi(prior_pose)), _dp(info)))

    def clear_pose_prior(self):
        self.set_pose_prior(None, None)

    def host_register(self, array: np.ndarray):
        self._check(self._lib.vgicp_host_register(self._h, array.ctypes.data, array.nbytes))

    def host_unregister(self, array: np.ndarray):
        self._check(self._lib.vgicp_host_unregister(self._h, array.ctypes.data))

    def scan_download(self):
        """The resident scan -> (points n x 3, covs n x 9)."""
        n = C.c_size_t(0)
        self._check(self._lib.vgicp_scan_download(self._h, 0, None, None, C.byref(n)))   # size query
        cap = n.value
        pts, covs = np.zeros((cap, 3)), np.zeros((cap, 9))
        self._check(self._lib.vgicp_scan_download(self._h, cap, _dp(pts), _dp(covs), C.byref(n)))
        return pts[:n.value], covs[:n.value]

    # -- multi-GPU --
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        self._check(self._lib.vgicp_comm_unique_id(self._h, buf))
        return buf.raw

    def comm_init(self, world_size: int, rank: int, unique_id: bytes):
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        buf = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        self._check(self._lib.vgicp_comm_init(self._h, int(world_size), int(rank), buf))

    def comm_destroy(self):
        self._check(self._lib.vgicp_comm_destroy(self._h))

    def peer_export(self) -> bytes:
        """IPC handle (64 bytes) of this context's mailbox for the device-initiated exchange."""
        buf = C.create_string_buffer(PEER_HANDLE_BYTES)
        self._check(self._lib.vgicp_peer_export(self._h, buf))
        return buf.raw

    def peer_connect(self, world_size: int, rank: int, handles: bytes):
        """handles: the world_size exported handles concatenated in rank order. The caller runs a barrier of its
        own transport after every rank has connected, before the first align."""
        if len(handles) != world_size * PEER_HANDLE_BYTES:
            raise ValueError("handles must hold world_size x 64 bytes")
        buf = C.create_string_buffer(handles, len(handles))
        self._check(self._lib.vgicp_peer_connect(self._h, int(world_size), int(rank), buf))

    def peer_disconnect(self):
        self._check(self._lib.vgicp_peer_disconnect(self._h))


def pose_prior_chart(prior_pose, pose):
    """vgicp_pose_prior_chart (vgicp_hip_prior.h), host only: (d (6), G (6 x 6)) of the prior's chart for `pose` against
    `prior_pose`, by the formulas the kernels use."""
    lib = load_library()
    d, G = np.zeros(6), np.zeros(36)
    rc = lib.vgicp_pose_prior_chart(_dp(pose_to_abi(prior_pose)), _dp(pose_to_abi(pose)), _dp(d), _dp(G))
    if rc != OK:
        raise VgicpError(rc, "vgicp_pose_prior_chart: a pose is missing or not finite")
    return d, G.reshape(6, 6).T.copy()


def posterior_information(normal_eq, prior_pose, pose, information):
    """G^-T A G^-1 + information: the information of `pose` in the filter's chart around prior_pose, from the data's
    normal equations at that pose (27 doubles as vgicp_stats.normal_eq lays them out: the xi chart) and the prior's."""
    A = np.zeros((6, 6))
    rows, cols = np.tril_indices(6)
    A[rows, cols] = np.asarray(normal_eq, dtype=np.float64)[:21]
    A = A + np.tril(A, -1).T
    _, G = pose_prior_chart(prior_pose, pose)
    G_inv = np.linalg.inv(G)
    return G_inv.T @ A @ G_inv + np.asarray(information, dtype=np.float64).reshape(6, 6)
