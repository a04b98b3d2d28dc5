#!/usr/bin/env python3
"""What vgicp_map_checkpoint and vgicp_map_restore (include/vgicp_hip_map_checkpoint.h) cost, beside the host routes that
were the only way to save and load a map before them and beside vgicp_scan_from_map of the whole map, which scans the same
table with the same three launches.  A developer tool, not a test; the pattern of tools/probe_map_submap.py, whose
frame-chain state it times on.

Three maps: the second frame's map of bench.py's frame chain (sweep 0 inserted) without and with the raw-point store, and
a C2-size map (synth.make_map(1 000 000), upserted) without.  Several processes one after the other, each under a time
limit of its own; per figure the median (p10 - p90) over the timed calls of all processes.

  checkpoint   vgicp_checkpoint_stats.device_seconds (the event span around the launches and the device-to-host copies
               into page-locked memory) and .seconds (the call's wall time: the one synchronisation, the checksum and the
               copy into the caller's buffer included)
  restore      likewise, into a second context: the span holds the table's clear, the host-to-device copies and the
               launches; the wall time also the check, the allocation of the new table (and log) and the release of the
               old ones, and the copy into page-locked memory.  Of these only the check is timed on its own
  check        vgicp_map_checkpoint_info of the blob: the checksum and the index rules, host only
  host routes  saving: vgicp_map_export (+ vgicp_map_points_export with the store); loading: vgicp_map_reset +
               vgicp_map_upsert (without the store only: a mirror batch carries no raw points), wall time
  from map     vgicp_scan_from_map of the whole map under the identity: device and wall time

    python tools/probe_map_checkpoint.py --out profiles/map_checkpoint_timing.txt
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
import probe_map_gated as frame  # noqa: E402

FIGURES = ("ckpt_dev", "ckpt_wall", "rest_dev", "rest_wall", "check", "save_host", "load_host", "from_dev", "from_wall")


def measure(capi, ctx, steps, warmup, host_steps, raw):
    voxels, slots = ctx.map_size()
    out = {k: [] for k in FIGURES}
    blob = ctx.map_checkpoint()
    st = ctx.last_checkpoint
    out.update(voxels=int(voxels), slots=int(slots), bytes=int(st.bytes), raw_points=int(st.raw_points), launches=int(st.launches))
    with capi.Context(0) as other:
        for step in range(warmup + steps):
            again = ctx.map_checkpoint()
            st = ctx.last_checkpoint
            rs = other.map_restore(blob)
            t0 = time.perf_counter()
            rule = capi.map_checkpoint_info(blob)["rule"]
            t1 = time.perf_counter()
            if rule != 0 or not np.array_equal(again, blob):
                raise SystemExit("a checkpoint changed, or fails the check")
            if step >= warmup:
                out["ckpt_dev"].append(st.device_seconds * 1e6)
                out["ckpt_wall"].append(st.seconds * 1e6)
                out["rest_dev"].append(rs.device_seconds * 1e6)
                out["rest_wall"].append(rs.seconds * 1e6)
                out["check"].append((t1 - t0) * 1e6)
        out["restore_launches"] = int(rs.launches)
        if not np.array_equal(other.map_checkpoint(), blob):
            raise SystemExit("the restored map's checkpoint is not the blob")
        for step in range(2 + host_steps):
            t0 = time.perf_counter()
            exported = ctx.map_export()
            if raw:
                ctx.map_points_export()
            t1 = time.perf_counter()
            if not raw:
                other.map_reset(ctx_voxel(ctx, blob), voxels)
                other.map_upsert(*exported[:3])
            t2 = time.perf_counter()
            if step >= 2:
                out["save_host"].append((t1 - t0) * 1e6)
                if not raw:
                    out["load_host"].append((t2 - t1) * 1e6)
    for step in range(warmup + steps):
        s = ctx.scan_from_map(ctx, (0.0, 0.0, 0.0), math.inf)
        if step >= warmup:
            out["from_dev"].append(s.device_seconds * 1e6)
            out["from_wall"].append(s.seconds * 1e6)
    return out


def ctx_voxel(ctx, blob):
    return float(np.asarray(blob[24:32]).view("<f8")[0])


def worker(steps, warmup, host_steps):
    from eskf_lio_amd import capi, synth
    result = {}
    sweeps, tt, st, ext = frame.inputs()
    for name, raw in (("frame", False), ("frame_raw", True)):
        with capi.Context(0) as ctx:
            dev, cus, _ = ctx.device_info()
            result["device"] = f"{dev}, {cus} compute units"
            if raw:
                ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
            ctx.map_reset(frame.VOXEL, 400_000)
            ctx.scan_prepare(sweeps[0], tt, st, ext, frame.VOXEL, frame.KNN)
            ctx.map_insert_resident(np.eye(4), frame.CAP)
            result[name] = measure(capi, ctx, steps, warmup, host_steps, raw)
    vmap = synth.make_map(1_000_000)
    with capi.Context(0) as ctx:
        ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0])
        ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
        result["c2"] = measure(capi, ctx, max(5, steps // 10), 2, max(3, host_steps // 5), False)
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
    return f"{np.median(d):11.1f} ({np.percentile(d, 10):11.1f} - {np.percentile(d, 90):11.1f})"


def report(title, runs, raw):
    r = runs[0]
    pooled = {k: [v for run in runs for v in run[k]] for k in FIGURES}
    med = {k: float(np.median(v)) if v else float("nan") for k, v in pooled.items()}
    lines = [f"{title}: {r['voxels']} voxels in {r['slots']} slots, a blob of {r['bytes']} bytes" +
             (f" with {r['raw_points']} raw points" if raw else ""),
             f"   vgicp_map_checkpoint ({r['launches']} launches), device span   {figure(pooled['ckpt_dev'])} us   ({len(pooled['ckpt_dev'])} calls)",
             f"   vgicp_map_checkpoint, wall                     {figure(pooled['ckpt_wall'])} us",
             f"      outside the span (checksum, copy to the caller): {100.0 * (med['ckpt_wall'] - med['ckpt_dev']) / med['ckpt_wall']:.0f} % of the wall time; "
             f"the span beyond the from-map scan's (mostly the copies over PCIe): {100.0 * max(0.0, med['ckpt_dev'] - med['from_dev']) / med['ckpt_wall']:.0f} %",
             f"   vgicp_map_restore ({r['restore_launches']} launches), device span      {figure(pooled['rest_dev'])} us",
             f"   vgicp_map_restore, wall                        {figure(pooled['rest_wall'])} us",
             f"      outside the span (the check, the allocation of the new table and the release of the old, the copy into page-locked memory; "
             f"only the check is timed on its own, below): {100.0 * (med['rest_wall'] - med['rest_dev']) / med['rest_wall']:.0f} % of the wall time",
             f"   the check alone (checksum and index rules)     {figure(pooled['check'])} us = {100.0 * med['check'] / med['rest_wall']:.0f} % of a restore's wall time",
             f"   host route, saving: vgicp_map_export" + (" + vgicp_map_points_export" if raw else "") +
             f", wall   {figure(pooled['save_host'])} us   ({len(pooled['save_host'])} rounds) = the checkpoint's wall x {med['save_host'] / med['ckpt_wall']:.1f}"]
    if raw:
        lines.append("   host route, loading: none (vgicp_map_upsert is refused while the map keeps raw points)")
    else:
        lines.append(f"   host route, loading: vgicp_map_reset + vgicp_map_upsert, wall   {figure(pooled['load_host'])} us = the restore's wall x "
                     f"{med['load_host'] / med['rest_wall']:.1f}")
    lines += [f"   vgicp_scan_from_map of the whole map, device   {figure(pooled['from_dev'])} us   ({len(pooled['from_dev'])} calls)",
              f"   vgicp_scan_from_map of the whole map, wall     {figure(pooled['from_wall'])} us"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=15)
    ap.add_argument("--limit", type=int, default=240, help="seconds a measuring process may take")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.warmup, a.host_steps)
        return
    from eskf_lio_amd import capi
    load0 = os.getloadavg()
    runs = [run_child(a.steps, a.warmup, a.host_steps, a.limit) for _ in range(a.processes)]
    load1 = os.getloadavg()
    lines = [f"tools/probe_map_checkpoint.py: {a.processes} processes one after the other, each {a.steps} timed calls after {a.warmup} per device "
             f"figure and {a.host_steps} rounds after 2 per host figure (a tenth and a fifth on the C2 map), us, median (p10 - p90) over all",
             f"one box: {runs[0]['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"library sha256 {frame.sha256(capi.LIB_PATH)}", ""]
    lines += report("1. the second frame's map of bench.py's frame chain, raw points off", [r["frame"] for r in runs], False) + [""]
    lines += report("2. the same map, raw points on", [r["frame_raw"] for r in runs], True) + [""]
    lines += report("3. a C2-size map, raw points off", [r["c2"] for r in runs], False)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
