"""Python handles on the C++ host mirror (libvgicp_host.so = include/eskf_lio_shim/ compiled).

`LocalMap` and `ICP` here are thin ctypes proxies of the C++ classes ESKF_LIO::LocalMap and
ESKF_LIO::ICP that keep the reference's method names and argument meaning (reference
include/ESKF_LIO/LocalMap.hpp:91-98, include/ESKF_LIO/Registration.hpp:23-32), so parity tests read
like tests of the reference would: build a map with updateLocalMap(), register with align().
No compute happens in Python and there is no fallback: errors of the HIP module surface as
RuntimeError with the library's message.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libvgicp_host.so")
_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    capi.load_library()  # libvgicp_hip.so first (RTLD_GLOBAL), the host layer links against it
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() / make -C eskf_lio_amd/host")
    lib = C.CDLL(LIB_PATH)
    vp, dp, sz = C.c_void_p, C.POINTER(C.c_double), C.c_size_t
    lib.host_last_error.restype = C.c_char_p
    lib.host_localmap_create_config.restype = vp
    lib.host_localmap_create_config.argtypes = [C.c_double, sz, C.c_double, C.c_double, C.c_int, C.c_double,
                                                C.c_double, C.c_int, C.c_int]
    lib.host_localmap_create_config_raw.restype = vp
    lib.host_localmap_create_config_raw.argtypes = [C.c_double, sz, C.c_double, C.c_double, C.c_int, C.c_double,
                                                    C.c_double, C.c_int, C.c_int, C.c_int]
    lib.host_localmap_saves_raw_points.restype = C.c_int
    lib.host_localmap_saves_raw_points.argtypes = [vp]
    lib.host_localmap_create.restype = vp
    lib.host_localmap_create.argtypes = [C.c_double, sz]
    lib.host_localmap_destroy.argtypes = [vp]
    lib.host_localmap_size.restype = sz
    lib.host_localmap_size.argtypes = [vp]
    lib.host_hash_helpers.restype = None
    lib.host_hash_helpers.argtypes = [C.c_int]
    lib.host_localmap_drain.restype = sz
    lib.host_localmap_drain.argtypes = [vp]
    lib.host_localmap_update.argtypes = [vp, sz, dp, dp, dp, C.c_int]
    lib.host_localmap_set_insert_gate.argtypes = [vp, C.c_double]
    lib.host_localmap_insert_gate.restype = C.c_double
    lib.host_localmap_insert_gate.argtypes = [vp]
    lib.host_localmap_gated_totals.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.host_localmap_set_carve.argtypes = [vp, C.c_double, C.c_double, C.c_uint32, C.c_uint32, dp]
    lib.host_localmap_clear_carve.restype = None
    lib.host_localmap_clear_carve.argtypes = [vp]
    lib.host_localmap_carve_totals.argtypes = [vp, C.POINTER(C.c_uint64)]
    u64p = C.POINTER(C.c_uint64)
    lib.host_localmap_ray_report.argtypes = [vp, dp, dp, C.c_uint32, sz, C.POINTER(C.c_uint8), dp, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_uint32), u64p, C.POINTER(sz), C.POINTER(C.c_int)]
    lib.host_localmap_ray_counts.argtypes = [vp, sz, dp, dp, C.c_uint32, u64p, C.POINTER(C.c_int)]
    lib.host_localmap_match.argtypes = [vp, sz, dp, dp, dp, dp, dp, dp, C.POINTER(sz)]
    lib.host_localmap_export.restype = sz
    lib.host_localmap_export.argtypes = [vp, sz, C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_uint64)]
    lib.host_localmap_save.argtypes = [vp, C.c_char_p, C.c_char_p]
    lib.host_localmap_counter.restype = C.c_uint64
    lib.host_localmap_counter.argtypes = [vp, C.c_int]
    lib.host_icp_create.restype = vp
    lib.host_icp_create.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int]
    lib.host_icp_create_robust.restype = vp
    lib.host_icp_create_robust.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.c_char_p, C.c_double, C.c_double]
    lib.host_icp_set_robust.argtypes = [vp, C.c_int, C.c_double, C.c_double, dp]
    lib.host_icp_hypotheses_per_launch.argtypes = [vp]
    lib.host_icp_align_with_prior.argtypes = [vp, sz, dp, dp, vp, dp, dp, dp, dp, C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.host_icp_destroy.argtypes = [vp]
    lib.host_icp_align.argtypes = [vp, sz, dp, dp, vp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_uint64), sz]
    i32p, u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    lib.host_icp_align_hypotheses.argtypes = [vp, sz, dp, dp, vp, sz, dp, dp, i32p, i32p, u64p, i32p, dp, i32p]
    lib.host_frame_hypotheses.argtypes = [vp, vp, vp, vp, sz, dp, dp, i32p, i32p, u64p, i32p, i32p]
    lib.host_icp_evaluate.argtypes = [vp, sz, dp, dp, vp, sz, dp, dp, i32p]
    lib.host_icp_align_best_by_score.argtypes = [vp, sz, dp, dp, vp, sz, dp, i32p, dp, i32p, i32p, dp]
    lib.host_frame_evaluate.argtypes = [vp, vp, vp, vp, sz, dp, C.c_int, dp, i32p]
    u8p = C.POINTER(C.c_uint8)
    lib.host_icp_point_report.argtypes = [vp, sz, dp, dp, vp, dp, sz, dp, C.c_int, sz, dp, dp, dp, u8p, u64p, dp, i32p]
    lib.host_frame_point_report.argtypes = [vp, vp, vp, vp, dp, sz, dp, C.c_int, sz, dp, dp, dp, u8p, u64p, dp, i32p]
    lib.host_icp_robust_scale_from_quantile.argtypes = [C.c_double, C.c_double, dp]
    lib.host_preprocessor_create.restype = vp
    lib.host_preprocessor_create.argtypes = [C.c_double, dp, C.c_int, C.c_int]
    lib.host_frame_begin.restype = vp
    lib.host_frame_begin.argtypes = [sz, dp, dp, sz, dp]
    lib.host_frame_run.argtypes = [vp, vp, vp, vp, dp, C.c_int, C.c_int, vp, C.c_int]
    lib.host_frame_stage.argtypes = [vp, vp]
    lib.host_frame_stage.restype = C.c_int
    lib.host_frame_end.argtypes = [vp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                   C.POINTER(sz), sz, dp, dp]
    lib.host_preprocessor_process.argtypes = [vp, sz, dp, dp, sz, dp, dp, dp, C.POINTER(sz)]
    lib.host_preprocessor_destroy.argtypes = [vp]
    lib.host_preprocessor_downsample.argtypes = [vp, sz, dp, dp, dp, C.POINTER(sz)]
    lib.host_math_ldlt6_solve.argtypes = [dp, dp, dp]
    lib.host_math_ldlt6_solve.restype = None
    lib.host_math_se3_exp.argtypes = [dp, dp]
    lib.host_math_se3_exp.restype = None
    _lib = lib
    return lib


def math_ldlt6_solve(JTJ, b) -> np.ndarray:
    """csrc/vgicp_math.h's pivoted LDLT (the kernels' solve) compiled for the host: A x = b with A a
    6x6 (row, col) array of which the lower triangle is read."""
    A = np.asarray(JTJ, dtype=np.float64).reshape(6, 6)
    low = np.ascontiguousarray([A[r, c] for r in range(6) for c in range(r + 1)], dtype=np.float64)
    rhs = np.ascontiguousarray(b, dtype=np.float64).reshape(6)
    x = np.zeros(6)
    load_library().host_math_ldlt6_solve(_dp(low), _dp(rhs), _dp(x))
    return x


def math_se3_exp(xi) -> np.ndarray:
    v = np.ascontiguousarray(xi, dtype=np.float64).reshape(6)
    out = np.zeros(16)
    load_library().host_math_se3_exp(_dp(v), _dp(out))
    return out.reshape(4, 4).T.copy()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _check(lib, rc):
    if rc != 0:
        raise RuntimeError(lib.host_last_error().decode())


class LocalMap:
    """ESKF_LIO::LocalMap.  config: the YAML keys + device_resident (default True: the grid the registration reads lives
    on the device) + keep_raw_points (default True: a host-side shadow grid keeps every raw point for save()) +
    raw_points_on_device (default False: with the two above, the device map keeps the raw points instead of the
    shadow grid, LocalMapConfig::rawPointsOnDevice)."""

    def __init__(self, voxelSize: float, maxNumPointsPerVoxel: int, config: Optional[dict] = None):
        self._lib = load_library()
        if config is None:
            self._h = self._lib.host_localmap_create(float(voxelSize), int(maxNumPointsPerVoxel))
        else:
            args = (float(voxelSize), int(maxNumPointsPerVoxel), float(config["translation_sq_threshold"]),
                    float(config["cosine_threshold"]), int(bool(config["remove_distant_points"])),
                    float(config["distance_threshold"]), float(config["removing_period"]),
                    int(bool(config.get("device_resident", True))), int(bool(config.get("keep_raw_points", True))))
            if "raw_points_on_device" in config:
                self._h = self._lib.host_localmap_create_config_raw(*args, int(bool(config["raw_points_on_device"])))
            else:
                self._h = self._lib.host_localmap_create_config(*args)
        if not self._h:
            raise RuntimeError(self._lib.host_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.host_localmap_destroy(self._h)
            self._h = None

    def __len__(self):
        return self._lib.host_localmap_size(self._h)

    def savesRawPoints(self) -> bool:
        """True while save() writes every stored raw point, as the reference does."""
        return bool(self._lib.host_localmap_saves_raw_points(self._h))

    def setInsertGate(self, gate: float):
        """LocalMap::setInsertGate: 0 = off; > 0 keeps the points that fail max(d^2, 0) <= gate out of the map."""
        if self._lib.host_localmap_set_insert_gate(self._h, float(gate)) != 0:
            raise ValueError(self._lib.host_last_error().decode())

    def insertGate(self) -> float:
        return float(self._lib.host_localmap_insert_gate(self._h))

    def gatedTotals(self):
        """(points the gated insertions saw, points they refused, frames inserted whole while a gate was set)."""
        out = (C.c_uint64 * 3)()
        _check(self._lib, self._lib.host_localmap_gated_totals(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def setCarve(self, margin: float = 0.0, max_range: float = 80.0, min_hits: int = 1, stride: int = 1,
                 origin=(0.0, 0.0, 0.0)):
        """LocalMap::setCarve (vgicp_hip_map_carve.h): every update on the resident scan first removes the voxels that
        scan sees through.  origin: the sensor's origin in the prepared scan's frame (the extrinsic's translation)."""
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        if not (0 <= int(min_hits) < 2 ** 32 and 0 <= int(stride) < 2 ** 32):
            raise ValueError("LocalMap::setCarve: min_hits and stride are 32-bit counts")
        if self._lib.host_localmap_set_carve(self._h, float(margin), float(max_range), int(min_hits), int(stride), _dp(o)) != 0:
            raise ValueError(self._lib.host_last_error().decode())

    def clearCarve(self):
        self._lib.host_localmap_clear_carve(self._h)

    def carveTotals(self):
        """(rays cast, voxels removed) by this map's carving since it was made."""
        out = (C.c_uint64 * 2)()
        _check(self._lib, self._lib.host_localmap_carve_totals(self._h, out))
        return int(out[0]), int(out[1])

    @staticmethod
    def _ray_params(margin, beyond, max_range, origin):
        return np.ascontiguousarray([*[float(v) for v in origin], float(margin), float(beyond), float(max_range)], dtype=np.float64)

    @staticmethod
    def _ray_counts(words):
        return dict(rays=int(words[0]), visits=int(words[1]), by_class=[int(v) for v in words[2:10]])

    def rayReport(self, transform, margin: float = 0.0, beyond: float = 0.0, max_range: float = 80.0, stride: int = 1,
                  origin=(0.0, 0.0, 0.0)):
        """LocalMap::rayReport (vgicp_hip_map_rays.h): the first map voxel on every ray of the resident scan at
        `transform`, read-only.  None where the map or the scan is not on the device; else a dict of status, range,
        hit_key, steps and counts."""
        T = capi.pose_to_abi(transform)
        p = self._ray_params(margin, beyond, max_range, origin)
        n, available, counts = C.c_size_t(0), C.c_int(0), (C.c_uint64 * 10)()
        # the size first, then the planes
        _check(self._lib, self._lib.host_localmap_ray_report(self._h, _dp(T), _dp(p), int(stride), 0, None, None, None, None,
                                                             counts, C.byref(n), C.byref(available)))
        if not available.value:
            return None
        m = n.value
        status, rng = np.zeros(m, dtype=np.uint8), np.zeros(m)
        keys, steps = np.zeros((m, 3), dtype=np.int32), np.zeros(m, dtype=np.uint32)
        _check(self._lib, self._lib.host_localmap_ray_report(
            self._h, _dp(T), _dp(p), int(stride), m, status.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(rng),
            keys.ctypes.data_as(C.POINTER(C.c_int32)), steps.ctypes.data_as(C.POINTER(C.c_uint32)), counts, C.byref(n),
            C.byref(available)))
        if not available.value or n.value != m:
            return None
        return dict(status=status, range=rng, hit_key=keys, steps=steps, counts=self._ray_counts(counts))

    def rayCounts(self, transforms, margin: float = 0.0, beyond: float = 0.0, max_range: float = 80.0, stride: int = 1,
                  origin=(0.0, 0.0, 0.0)):
        """LocalMap::rayCounts: the counts alone at several poses (at most 64); None where not available."""
        Ts = np.ascontiguousarray(np.stack([capi.pose_to_abi(T) for T in transforms]).reshape(-1, 16))
        p = self._ray_params(margin, beyond, max_range, origin)
        available, counts = C.c_int(0), (C.c_uint64 * (10 * len(Ts)))()
        _check(self._lib, self._lib.host_localmap_ray_counts(self._h, len(Ts), _dp(Ts), _dp(p), int(stride), counts,
                                                             C.byref(available)))
        return [self._ray_counts(counts[10 * k:10 * k + 10]) for k in range(len(Ts))] if available.value else None

    def drain(self) -> int:
        """Waits for the shadow grid's worker (LocalMap::grid()); the host grid's voxel count."""
        return self._lib.host_localmap_drain(self._h)

    def updateLocalMap(self, points, covs, transform, initialize: bool = False):
        """Returns the cloud moved into the world frame (the reference mutates it in place)."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3).copy()
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9).copy()
        T = capi.pose_to_abi(transform)
        _check(self._lib, self._lib.host_localmap_update(self._h, pts.shape[0], _dp(pts), _dp(cvs), _dp(T),
                                                         int(initialize)))
        return pts, cvs

    def correspondenceMatching(self, points, covs):
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9)
        n = pts.shape[0]
        sp, sc, mp, mc = np.zeros((n, 3)), np.zeros((n, 9)), np.zeros((n, 3)), np.zeros((n, 9))
        m = C.c_size_t()
        _check(self._lib, self._lib.host_localmap_match(self._h, n, _dp(pts), _dp(cvs), _dp(sp), _dp(sc),
                                                        _dp(mp), _dp(mc), C.byref(m)))
        k = m.value
        return sp[:k], sc[:k], mp[:k], mc[:k]

    def export(self):
        n = len(self)
        keys = np.zeros((n, 3), dtype=np.int32)
        means, covs = np.zeros((n, 3)), np.zeros((n, 9))
        counts = np.zeros(n, dtype=np.uint64)
        w = self._lib.host_localmap_export(self._h, n, keys.ctypes.data_as(C.POINTER(C.c_int32)), _dp(means),
                                           _dp(covs), counts.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert w == n
        return keys, means, covs, counts

    def counter(self, which: int) -> int:
        """vgicp_get_counter of the map's device context (capi.Context.counter)."""
        return int(self._lib.host_localmap_counter(self._h, int(which)))

    def save(self, cloud_path: str, trajectory_path: str):
        _check(self._lib, self._lib.host_localmap_save(self._h, cloud_path.encode(), trajectory_path.encode()))


class ICP:
    """ESKF_LIO::ICP: config keys as in registration.* of the reference's YAML."""

    def __init__(self, max_iteration: int, translation_sq_threshold: float, cosine_threshold: float,
                 chunk_iterations: int = 0, robust_kernel: Optional[str] = None, robust_scale: float = 1.0,
                 gate: float = 0.0):
        """robust_kernel ("none" / "huber" / "cauchy"), robust_scale, gate: the optional keys of registration.* that
        switch the robust round on (vgicp_hip_robust.h); absent = the reference's plain least squares."""
        self._lib = load_library()
        self.max_iteration = int(max_iteration)
        if robust_kernel is None and robust_scale == 1.0 and gate == 0.0:
            self._h = self._lib.host_icp_create(self.max_iteration, float(translation_sq_threshold),
                                                float(cosine_threshold), int(chunk_iterations))
        else:
            self._h = self._lib.host_icp_create_robust(
                self.max_iteration, float(translation_sq_threshold), float(cosine_threshold), int(chunk_iterations),
                None if robust_kernel is None else str(robust_kernel).encode(), float(robust_scale), float(gate))
            if not self._h:
                raise ValueError(self._lib.host_last_error().decode())
        self.iterations = 0
        self.converged = False
        self.correspondence_counts = np.zeros(0, dtype=np.uint64)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.host_icp_destroy(self._h)
            self._h = None

    def setRobust(self, kind: int, scale: float, gate: float):
        """ICP::setRobust -> (kind, scale, gate) as the library will use them; ValueError for what it refuses."""
        out = np.zeros(3)
        if self._lib.host_icp_set_robust(self._h, int(kind), float(scale), float(gate), _dp(out)) != 0:
            raise ValueError(self._lib.host_last_error().decode())
        return int(out[0]), float(out[1]), float(out[2])

    @property
    def hypotheses_per_launch(self) -> int:
        """ICP::lastHypothesesPerLaunch(): of the last alignHypotheses; 1 = one by one."""
        return int(self._lib.host_icp_hypotheses_per_launch(self._h))

    def align(self, points, covs, localMap: LocalMap, guess) -> np.ndarray:
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9)
        g = capi.pose_to_abi(guess)
        out = np.zeros(16)
        it, conv = C.c_int32(), C.c_int32()
        cap = max(self.max_iteration, 1)
        counts = np.zeros(cap, dtype=np.uint64)
        _check(self._lib, self._lib.host_icp_align(self._h, pts.shape[0], _dp(pts), _dp(cvs), localMap._h, _dp(g),
                                                   _dp(out), C.byref(it), C.byref(conv),
                                                   counts.ctypes.data_as(C.POINTER(C.c_uint64)), cap))
        self.iterations, self.converged = it.value, bool(conv.value)
        self.correspondence_counts = counts[:it.value].copy()
        return capi.pose_from_abi(out)

    def alignWithPrior(self, points, covs, localMap: LocalMap, guess, information) -> np.ndarray:
        """ICP::alignWithPrior (vgicp_hip_prior.h): the MAP pose of the cloud given the pose `guess` with the 6 x 6
        `information` in the filter's chart; posteriorInformation() then has the returned pose's information."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9)
        g = capi.pose_to_abi(guess)
        info = np.ascontiguousarray(np.asarray(information, dtype=np.float64).reshape(6, 6).T).reshape(36)
        out, post = np.zeros(16), np.zeros(36)
        it, conv, left = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self._lib, self._lib.host_icp_align_with_prior(self._h, pts.shape[0], _dp(pts), _dp(cvs), localMap._h,
                                                              _dp(g), _dp(info), _dp(out), _dp(post), C.byref(it),
                                                              C.byref(conv), C.byref(left)))
        self.iterations, self.converged = it.value, bool(conv.value)
        self.prior_left_behind = bool(left.value)
        self._posterior = post.reshape(6, 6).T.copy()
        return capi.pose_from_abi(out)

    def posteriorInformation(self) -> np.ndarray:
        """ICP::posteriorInformation of the last alignWithPrior: G^-T A G^-1 + information, 6 x 6."""
        return self._posterior.copy()

    def alignHypotheses(self, points, covs, localMap: LocalMap, guesses):
        """ICP::alignHypotheses on a cloud made from the arrays (one upload) -> [dict(pose, converged, iterations,
        finalCorrespondences)], one per guess."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9)
        g, out, it, conv, fin = _fan_buffers(guesses)
        res = C.c_int32()
        _check(self._lib, self._lib.host_icp_align_hypotheses(
            self._h, pts.shape[0], _dp(pts), _dp(cvs), localMap._h, g.shape[0], _dp(g), _dp(out), _i32(it), _i32(conv),
            fin.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, C.byref(res)))
        self.used_resident = bool(res.value)
        return _fan_results(out, it, conv, fin)

    def alignBest(self, points, covs, localMap: LocalMap, guesses) -> np.ndarray:
        """ICP::alignBest -> the chosen pose; self.best is the chosen index, self.iterations / self.converged describe
        that hypothesis."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9)
        g, _, it, conv, _ = _fan_buffers(guesses)
        best, pose = C.c_int32(-1), np.zeros(16)
        _check(self._lib, self._lib.host_icp_align_hypotheses(
            self._h, pts.shape[0], _dp(pts), _dp(cvs), localMap._h, g.shape[0], _dp(g), None, _i32(it), _i32(conv), None,
            C.byref(best), _dp(pose), None))
        self.best, self.iterations, self.converged = int(best.value), int(it[0]), bool(conv[0])
        return capi.pose_from_abi(pose)

    def evaluate(self, points, covs, localMap: LocalMap, poses):
        """ICP::evaluate on a cloud made from the arrays (one upload) -> [capi.PoseEvaluation], one per pose."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9)
        g = _fan_buffers(poses)[0]
        out = np.zeros((g.shape[0], 31))
        res = C.c_int32()
        _check(self._lib, self._lib.host_icp_evaluate(self._h, pts.shape[0], _dp(pts), _dp(cvs), localMap._h,
                                                      g.shape[0], _dp(g), _dp(out), C.byref(res)))
        self.used_resident = bool(res.value)
        return [_evaluation(row) for row in out]

    def pointReport(self, points, covs, localMap: LocalMap, pose, quantiles=(), perPoint: bool = True):
        """ICP::pointReport on a cloud made from the arrays (one upload) -> capi.PointReport."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9)
        buf = _PointReportBuffers(pts.shape[0], quantiles, perPoint)
        T = capi.pose_to_abi(pose)
        res = C.c_int32(0)
        _check(self._lib, self._lib.host_icp_point_report(self._h, pts.shape[0], _dp(pts), _dp(cvs), localMap._h, _dp(T),
                                                          *buf.args(), C.byref(res)))
        self.used_resident = bool(res.value)
        return buf.report()

    @staticmethod
    def robustScaleFromQuantile(d2_quantile: float, factor: float = 1.0) -> float:
        """ICP::robustScaleFromQuantile: factor * sqrt(d2_quantile); ValueError for what it refuses."""
        lib = load_library()
        out = np.zeros(1)
        if lib.host_icp_robust_scale_from_quantile(float(d2_quantile), float(factor), _dp(out)) != 0:
            raise ValueError(lib.host_last_error().decode())
        return float(out[0])

    def alignBestByScore(self, points, covs, localMap: LocalMap, guesses) -> np.ndarray:
        """ICP::alignBestByScore -> the chosen pose; self.best is the chosen index, self.iterations / self.converged
        describe that hypothesis and self.evaluation is ICP::lastEvaluation()."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cvs = np.ascontiguousarray(covs, dtype=np.float64).reshape(-1, 9)
        g = _fan_buffers(guesses)[0]
        best, pose, it, conv, ev = C.c_int32(-1), np.zeros(16), C.c_int32(), C.c_int32(), np.zeros(31)
        _check(self._lib, self._lib.host_icp_align_best_by_score(
            self._h, pts.shape[0], _dp(pts), _dp(cvs), localMap._h, g.shape[0], _dp(g), C.byref(best), _dp(pose),
            C.byref(it), C.byref(conv), _dp(ev)))
        self.best, self.iterations, self.converged = int(best.value), int(it.value), bool(conv.value)
        self.evaluation = _evaluation(ev)
        return capi.pose_from_abi(pose)


class _PointReportBuffers:
    """The output arrays of host_icp_point_report / host_frame_point_report for a cloud of at most `capacity` points."""

    def __init__(self, capacity: int, quantiles, per_point: bool):
        self.q = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        self.per_point, self.capacity = bool(per_point), int(capacity) if per_point else 0
        self.d2, self.sq, self.w = (np.zeros(self.capacity) for _ in range(3))
        self.status = np.zeros(self.capacity, dtype=np.uint8)
        self.counts = np.zeros(5, dtype=np.uint64)
        self.quantiles = np.zeros(max(self.q.size, 1))

    def args(self):
        give = self.per_point and self.capacity > 0
        return (self.q.size, _dp(self.q) if self.q.size else None, 1 if self.per_point else 0, self.capacity,
                _dp(self.d2) if give else None, _dp(self.sq) if give else None, _dp(self.w) if give else None,
                self.status.ctypes.data_as(C.POINTER(C.c_uint8)) if give else None,
                self.counts.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(self.quantiles))

    def report(self) -> "capi.PointReport":
        n = min(int(self.counts[0]), self.capacity)
        cut = (lambda a: a[:n].copy()) if self.per_point else (lambda a: None)
        return capi.PointReport(points=int(self.counts[0]), matched=int(self.counts[1]), counted=int(self.counts[2]),
                                negative=int(self.counts[3]), not_finite=int(self.counts[4]),
                                quantiles=self.quantiles[:self.q.size].copy(), d2=cut(self.d2), sq_error=cut(self.sq),
                                weight=cut(self.w), status=cut(self.status))


def _evaluation(row) -> "capi.PoseEvaluation":
    """31 doubles of vgicp_host.cpp's packEvaluation -> capi.PoseEvaluation."""
    return capi.PoseEvaluation(points=int(row[0]), correspondences=int(row[1]), cost=float(row[2]),
                               sq_error=float(row[3]), normal_eq=np.array(row[4:31], dtype=np.float64))


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _fan_buffers(guesses):
    g = np.ascontiguousarray(np.stack([capi.pose_to_abi(T) for T in guesses]).reshape(-1, 16))
    k = g.shape[0]
    return g, np.zeros((k, 16)), np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.uint64)


def _fan_results(out, it, conv, fin):
    return [dict(pose=capi.pose_from_abi(out[h]), converged=bool(conv[h]), iterations=int(it[h]),
                 finalCorrespondences=int(fin[h])) for h in range(out.shape[0])]


class CloudPreprocessor:
    """ESKF_LIO::CloudPreprocessor's scan-preparation half (include/eskf_lio_shim/CloudPreprocessor.hpp;
    reference include/ESKF_LIO/CloudPreprocessor.hpp:35-36, src/CloudPreprocessor.cpp:76-127)."""

    def __init__(self, voxel_size: float, T_il=None, host_copy: Optional[str] = None, resident_check: str = "full"):
        """host_copy: "eager" (process() leaves the prepared scan in the host cloud, as the reference does),
        "deferred" (it stays on the device until somebody materialises it), None = the shim's default.
        resident_check: "full" (default: every byte of the host cloud is hashed before the resident scan is trusted) or
        "sampled" (CloudPreprocessorConfig::residentCheck = Sampled)."""
        self._lib = load_library()
        t = capi.pose_to_abi(np.eye(4) if T_il is None else T_il)
        mode = {None: -1, "eager": 0, "deferred": 1}[host_copy]
        self._h = self._lib.host_preprocessor_create(float(voxel_size), _dp(t), mode, 1 if resident_check == "sampled" else 0)
        if not self._h:
            raise RuntimeError(self._lib.host_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.host_preprocessor_destroy(self._h)
            self._h = None

    def voxelDownsampleAndEstimateCovariances(self, points):
        """cloud.points_ in -> (cloud.points_, cloud.covariances_) out."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        op, oc = np.zeros((n, 3)), np.zeros((n, 9))
        kept = C.c_size_t(0)
        _check(self._lib, self._lib.host_preprocessor_downsample(self._h, n, _dp(pts), _dp(op), _dp(oc),
                                                                 C.byref(kept)))
        return op[:kept.value].copy(), oc[:kept.value].copy()

    def process(self, states, points, pointTime):
        """process(states, lidarMeas): extrinsic -> deskew -> down-sampling + covariances
        (reference src/CloudPreprocessor.cpp:8-23). states: S x 8 (timestamp, position, quaternion xyzw)."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(pointTime, dtype=np.float64).reshape(-1)
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 8)
        n = pts.shape[0]
        op, oc = np.zeros((n, 3)), np.zeros((n, 9))
        kept = C.c_size_t(0)
        _check(self._lib, self._lib.host_preprocessor_process(self._h, n, _dp(pts), _dp(t), st.shape[0], _dp(st),
                                                              _dp(op), _dp(oc), C.byref(kept)))
        return op[:kept.value].copy(), oc[:kept.value].copy()


class Frame:
    """One LiDAR frame through the C++ drop-in classes the way src/Odometry.cpp:73-87 is written:
    process(states, meas) -> icp.align(*meas.cloud, localMap, guess) -> localMap.updateLocalMap(meas.cloud, T).
    begin (builds the measurement object) / run (the three calls; what a caller would time) / end (results)."""

    def __init__(self, points, pointTime, states):
        self._lib = load_library()
        self._pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self._t = np.ascontiguousarray(pointTime, dtype=np.float64).reshape(-1)
        self._st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 8)
        self._h = self._lib.host_frame_begin(self._pts.shape[0], _dp(self._pts), _dp(self._t), self._st.shape[0],
                                             _dp(self._st))

    def stage(self, preprocessor: "CloudPreprocessor") -> bool:
        """CloudPreprocessor::stage on this frame's measurement: what a lidar callback does when the sweep arrives."""
        rc = self._lib.host_frame_stage(self._h, preprocessor._h)
        if rc < 0:
            raise RuntimeError("CloudPreprocessor::stage failed")
        return bool(rc)

    def run(self, preprocessor: "CloudPreprocessor", icp: "ICP", localMap: "LocalMap", guess, first_frame=False,
            mutate: int = 0, stage_next: "Frame" = None, move_cloud: bool = False):
        """stage_next: a later Frame whose sweep 'arrives' during this one (staged right after this frame's process()).
        move_cloud: hand the cloud to updateLocalMap as src/Odometry.cpp:86 does (std::move: end() then has no cloud)."""
        g = capi.pose_to_abi(guess)
        _check(self._lib, self._lib.host_frame_run(self._h, preprocessor._h, icp._h, localMap._h, _dp(g),
                                                   1 if first_frame else 0, int(mutate),
                                                   stage_next._h if stage_next is not None else None, int(bool(move_cloud))))

    def evaluate(self, preprocessor: "CloudPreprocessor", icp: "ICP", localMap: "LocalMap", poses, mutate: int = 0):
        """process(states, meas), optionally an edit of the prepared cloud (mutate as run()), then ICP::evaluate on it
        (no map update) -> ([capi.PoseEvaluation], used_resident)."""
        g = _fan_buffers(poses)[0]
        out = np.zeros((g.shape[0], 31))
        res = C.c_int32()
        _check(self._lib, self._lib.host_frame_evaluate(self._h, preprocessor._h, icp._h, localMap._h, g.shape[0],
                                                        _dp(g), int(mutate), _dp(out), C.byref(res)))
        return [_evaluation(row) for row in out], bool(res.value)

    def pointReport(self, preprocessor: "CloudPreprocessor", icp: "ICP", localMap: "LocalMap", pose, quantiles=(),
                    perPoint: bool = True):
        """process(states, meas), then ICP::pointReport on the prepared cloud (no map update)
        -> (capi.PointReport, used_resident)."""
        buf = _PointReportBuffers(self._pts.shape[0], quantiles, perPoint)
        T = capi.pose_to_abi(pose)
        res = C.c_int32(0)
        _check(self._lib, self._lib.host_frame_point_report(self._h, preprocessor._h, icp._h, localMap._h, _dp(T),
                                                            *buf.args(), C.byref(res)))
        return buf.report(), bool(res.value)

    def hypotheses(self, preprocessor: "CloudPreprocessor", icp: "ICP", localMap: "LocalMap", guesses):
        """process(states, meas), then ICP::alignHypotheses on the cloud it left resident (no map update) ->
        (results as ICP.alignHypotheses, used_resident, hypotheses per launch)."""
        g, out, it, conv, fin = _fan_buffers(guesses)
        res, per = C.c_int32(), C.c_int32()
        _check(self._lib, self._lib.host_frame_hypotheses(
            self._h, preprocessor._h, icp._h, localMap._h, g.shape[0], _dp(g), _dp(out), _i32(it), _i32(conv),
            fin.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(res), C.byref(per)))
        return _fan_results(out, it, conv, fin), bool(res.value), int(per.value)

    def end(self, want_cloud: bool = False):
        """-> dict(pose, iterations, used_resident, corr0, host_points[, points, covs])."""
        out = np.zeros(16)
        it, res = C.c_int32(), C.c_int32()
        corr0 = C.c_uint64()
        hp = C.c_size_t()
        n = self._pts.shape[0]
        pts = np.zeros((n, 3)) if want_cloud else None
        cvs = np.zeros((n, 9)) if want_cloud else None
        _check(self._lib, self._lib.host_frame_end(self._h, _dp(out), C.byref(it), C.byref(res), C.byref(corr0),
                                                   C.byref(hp), n, _dp(pts) if want_cloud else None,
                                                   _dp(cvs) if want_cloud else None))
        self._h = None
        r = dict(pose=capi.pose_from_abi(out), iterations=it.value, used_resident=bool(res.value), corr0=int(corr0.value),
                 host_points=int(hp.value))
        if want_cloud:
            r["points"], r["covs"] = pts[:hp.value].copy(), cvs[:hp.value].copy()
        return r
