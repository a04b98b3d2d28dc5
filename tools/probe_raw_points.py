"""Developer probe: the raw-point store (VGICP_OPTION_MAP_RAW_POINTS) at the end of the 300-sweep street drive
(tests/golden/make_drive_fixture.py, the GPU-driven chain of eskf_lio_amd/replay.py's DeviceBackend): how many raw
points the map keeps, the store's size, and the time of vgicp_map_points_export for all of them (the C call alone,
five times; the caller's arrays allocated before)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from eskf_lio_amd import capi, replay  # noqa: E402
import make_drive_fixture as mk  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 300
cfg = mk.drive_config()
backend = replay.DeviceBackend(cfg, 0)
backend.ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
odo = replay.Odometry(cfg, backend)
t0 = time.perf_counter()
odo.run(mk.lazy_events(frames))
print(f"street drive, {frames} sweeps: {time.perf_counter() - t0:.1f} s")
ctx = backend.ctx
n, capacity = ctx.map_points_size()
voxels, slots = ctx.map_size()
counts = ctx.map_export()[3]
assert int(counts.sum()) == n
print(f"voxels {voxels} (table {slots} slots), raw points {n}, store capacity {capacity} entries "
      f"({capacity * 32 / 2**20:.0f} MiB)")
keys, pts, written = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 3)), C.c_size_t()
lib = capi.load_library()
ms = []
for _ in range(5):
    t = time.perf_counter()
    rc = lib.vgicp_map_points_export(ctx._h, n, keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                     pts.ctypes.data_as(C.POINTER(C.c_double)), C.byref(written))
    ms.append(1e3 * (time.perf_counter() - t))
    assert rc == 0 and written.value == n
print("vgicp_map_points_export, ms per call: " + " ".join(f"{x:.2f}" for x in ms))
