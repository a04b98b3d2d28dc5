#!/usr/bin/env python3
"""What vgicp_scan_from_map (include/vgicp_hip_map_submap.h) costs, beside the host route that gave the same scan before it
and beside a rebuild of level 1 on the same table.  A developer tool, not a test; the pattern of tools/probe_map_locate.py,
whose frame-chain state it times on.

Two maps: the second frame's map of bench.py's frame chain (sweep 0 inserted, levels 1 .. 2 kept) and a C2-size map
(synth.make_map(1 000 000), upserted).  One process under a time limit of its own; per figure the median (p10 - p90).

  device     vgicp_scan_from_map with radius = +inf, with a 20 m radius (frame chain; 10 m on C2) and on level 2 (frame
             chain only), each with a rotated frame: vgicp_submap_stats.device_seconds (the event span around the three
             launches) and .seconds (the call's wall time, its one synchronisation included)
  host       the same scan as the parent commit offers it, in the same process: vgicp_map_export (vgicp_map_level_export for
             the level) -> the selection and the transform in numpy (tests/map_submap_reference.py) -> vgicp_scan_upload;
             wall time of the three steps, and of the export and the upload alone.  The host route's scan comes in the
             export's order, which is unspecified
  level 1    vgicp_map_levels_build(1) after a change of the map: the clear of the level's table, the CLAIM launch over the
             map's table (the one pass over its slots that the MARK launch also makes) and the FILL launch, device time

    python tools/probe_map_submap.py --out profiles/map_submap_timing.txt
"""
import argparse
import json
import math
import os
import platform
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import probe_map_gated as frame  # noqa: E402


def rotated_frame():
    a = np.deg2rad(30.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (1.25, -0.5, 0.75)
    return T


def measure(ctx, cases, steps, warmup, host_steps, voxel):
    import map_submap_reference as ms
    T = rotated_frame()
    voxels, slots = ctx.map_size()
    out = dict(voxels=int(voxels), slots=int(slots), cases={})
    for name, center, radius, level in cases:
        dev, wall, st = [], [], None
        for step in range(warmup + steps):
            st = ctx.scan_from_map(ctx, center, radius, T, level=level)
            if st.launches != 3:
                raise SystemExit(f"a from-map call made {st.launches} launches")
            if step >= warmup:
                dev.append(st.device_seconds * 1e6)
                wall.append(st.seconds * 1e6)
        pts_dev = ctx.scan_download()[0]
        host, export, upload = [], [], []
        h = voxel * 2 ** level
        for step in range(2 + host_steps):
            t0 = time.perf_counter()
            exported = ctx.map_level_export(level) if level else ctx.map_export()
            t1 = time.perf_counter()
            sub = ms.submap(*exported, h, center, radius, T)
            t2 = time.perf_counter()
            ctx.scan_upload(sub.points, sub.covs)
            t3 = time.perf_counter()
            if step >= 2:
                host.append((t3 - t0) * 1e6)
                export.append((t1 - t0) * 1e6)
                upload.append((t3 - t2) * 1e6)
        if len(sub) != st.points or not np.array_equal(np.sort(pts_dev, axis=0), np.sort(sub.points, axis=0)):
            raise SystemExit(f"{name}: the two routes disagree")
        out["cases"][name] = dict(dev=dev, wall=wall, host=host, export=export, upload=upload, points=int(st.points),
                                  source=int(st.voxels))
    # a rebuild of level 1: one upsert of a voxel as it is bumps the map's version
    keys, means, covs, _ = ctx.map_export()
    build = []
    for step in range(3 + 30):
        ctx.map_upsert(keys[:1], means[:1], covs[:1])
        b = ctx.map_levels_build(max(1, ctx_levels(cases)))
        if step >= 3:
            build.append(b.device_seconds * 1e6)
    out["build"] = build
    out["build_levels"] = max(1, ctx_levels(cases))
    return out


def ctx_levels(cases):
    return max(level for _, _, _, level in cases)


def worker(steps, warmup, host_steps):
    from eskf_lio_amd import capi, synth
    result = {}
    sweeps, tt, st, ext = frame.inputs()
    with capi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        result["device"] = f"{name}, {cus} compute units"
        ctx.map_reset(frame.VOXEL, 400_000)
        ctx.scan_prepare(sweeps[0], tt, st, ext, frame.VOXEL, frame.KNN)
        ctx.map_insert_resident(np.eye(4), frame.CAP)
        ctx.map_levels_build(2)
        cases = (("radius +inf", (0.0, 0.0, 0.0), math.inf, 0), ("radius 20 m", (0.0, 0.0, 0.0), 20.0, 0),
                 ("level 2, radius +inf", (0.0, 0.0, 0.0), math.inf, 2))
        result["frame"] = measure(ctx, cases, steps, warmup, host_steps, frame.VOXEL)
    vmap = synth.make_map(1_000_000)
    with capi.Context(0) as ctx:
        ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0])
        ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
        ctx.map_levels_build(1)
        mid = tuple(float(v) for v in vmap.means.mean(axis=0))
        cases = (("radius +inf", mid, math.inf, 0), ("radius 10 m", mid, 10.0, 0))
        result["c2"] = measure(ctx, cases, steps, warmup, max(4, host_steps // 5), vmap.voxel_size)
    print("PROBE_RESULT " + json.dumps(result), flush=True)


def run_child(steps, warmup, host_steps, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(steps),
           "--warmup", str(warmup), "--host-steps", str(host_steps)]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
        raise SystemExit(f"child ended with status {proc.returncode}: nothing more is started")
    for line in proc.stdout.splitlines():
        if line.startswith("PROBE_RESULT "):
            return json.loads(line[len("PROBE_RESULT "):])
    raise SystemExit("child printed no result")


def figure(us):
    d = np.asarray(us, dtype=np.float64)
    return f"{np.median(d):10.1f} ({np.percentile(d, 10):10.1f} - {np.percentile(d, 90):10.1f})"


def report(name, r):
    lines = [f"{name}: {r['voxels']} voxels in {r['slots']} slots"]
    for case, c in r["cases"].items():
        lines.append(f"   {case}: {c['points']} points of {c['source']} voxels of the source table")
        lines.append(f"      vgicp_scan_from_map, device    {figure(c['dev'])} us   ({len(c['dev'])} calls)")
        lines.append(f"      vgicp_scan_from_map, wall      {figure(c['wall'])} us")
        lines.append(f"      host route, wall               {figure(c['host'])} us   ({len(c['host'])} rounds) = the device call's wall x "
                     f"{np.median(c['host']) / np.median(c['wall']):.0f}")
        lines.append(f"         of which the export         {figure(c['export'])} us")
        lines.append(f"         of which the upload         {figure(c['upload'])} us")
    lines.append(f"   vgicp_map_levels_build({r['build_levels']}) after a change of the map (clear, CLAIM, FILL per level), device   "
                 f"{figure(r['build'])} us   ({len(r['build'])} calls)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-steps", type=int, default=30)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.warmup, a.host_steps)
        return
    from eskf_lio_amd import capi
    load0 = os.getloadavg()
    r = run_child(a.steps, a.warmup, a.host_steps, a.limit)
    load1 = os.getloadavg()
    lines = [f"tools/probe_map_submap.py: one process, {a.steps} timed calls after {a.warmup} per device figure, {a.host_steps} rounds after 2 "
             f"per host figure (a fifth on the C2 map), us, median (p10 - p90)",
             f"one box: {r['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"library sha256 {frame.sha256(capi.LIB_PATH)}", ""]
    lines += report("1. the second frame's map of bench.py's frame chain", r["frame"]) + [""]
    lines += report("2. a C2-size map", r["c2"])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
