#!/usr/bin/env python3
"""What vgicp_map_merge (include/vgicp_hip_map_merge.h) costs, beside the two routes the parent commit offers towards the
same end.  A developer tool, not a test; the pattern of tools/probe_map_submap.py, whose frame-chain state it times on.

Two pairs of maps: the second frame's map of bench.py's frame chain (sweep 0 inserted) merged into a copy of itself
displaced by a frame, and a C2-size map (synth.make_map(1 000 000), upserted) likewise.  Several processes, each under a
time limit of its own, their samples pooled; per figure the median (p10 - p90).  Before every timed call the destination
is put back from a checkpoint (vgicp_map_restore, not timed), so that every call does the same work.

  merge      vgicp_map_merge(dst, src, whole map, rotated frame, max_count = the chain's cap): vgicp_merge_stats
             .device_seconds (the event span around its launches) and .seconds (the call's wall time, its one
             synchronisation included)
  insert     the parent's route on the device, which loses the counts: vgicp_scan_from_map(dst, src, the same frame) and
             vgicp_map_insert_resident(identity, the cap).  Wall: the two calls by the host's clock.  Device: the from-map
             call's device_seconds plus those of vgicp_map_insert_resident_gated with gate = +infinity on the same state —
             the plain insertion reports no device time; the gated one adds its decision launch to the insertion's
  exports    two vgicp_map_export calls (dst and src), the host's only way to the counts; nothing takes them back

    python tools/probe_map_merge.py --out profiles/map_merge_timing.txt
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
from probe_map_submap import rotated_frame  # noqa: E402


def measure(dst, src, steps, warmup, cap):
    T = rotated_frame()
    blob = dst.map_checkpoint()
    out = dict(voxels=int(src.map_size()[0]), slots=int(dst.map_size()[1]))
    dev, wall, launches, st = [], [], 0, None
    for step in range(warmup + steps):
        dst.map_restore(blob)
        st = dst.map_merge(src, frame=T, max_count=cap)
        if step >= warmup:
            dev.append(st.device_seconds * 1e6)
            wall.append(st.seconds * 1e6)
    out["merge"] = dict(dev=dev, wall=wall, launches=st.launches, created=st.created, updated=st.updated, frozen=st.frozen,
                        points=st.points, selected=st.selected)
    sub_dev, ins_dev, route_wall, new = [], [], [], 0
    for step in range(warmup + steps):
        dst.map_restore(blob)
        t0 = time.perf_counter()
        sub = dst.scan_from_map(src, (0.0, 0.0, 0.0), math.inf, T)
        new = dst.map_insert_resident(np.eye(4), cap)
        t1 = time.perf_counter()
        dst.map_restore(blob)
        _, gated = dst.map_insert_resident_gated(np.eye(4), cap, math.inf, kept=False)
        if step >= warmup:
            route_wall.append((t1 - t0) * 1e6)
            sub_dev.append(sub.device_seconds * 1e6)
            ins_dev.append(gated.device_seconds * 1e6)
    if new != st.created:
        raise SystemExit(f"the two routes open {st.created} and {new} voxels")
    out["insert"] = dict(wall=route_wall, sub_dev=sub_dev, ins_dev=ins_dev, sum_dev=[a + b for a, b in zip(sub_dev, ins_dev)])
    exports = []
    for step in range(2 + max(4, steps // 4)):
        t0 = time.perf_counter()
        dst.map_export()
        src.map_export()
        t1 = time.perf_counter()
        if step >= 2:
            exports.append((t1 - t0) * 1e6)
    out["exports"] = exports
    return out


def worker(steps, warmup):
    from eskf_lio_amd import capi, synth
    result = {}
    sweeps, tt, st, ext = frame.inputs()
    with capi.Context(0) as dst, capi.Context(0) as src:
        name, cus, _ = dst.device_info()
        result["device"] = f"{name}, {cus} compute units"
        for ctx in (dst, src):
            ctx.map_reset(frame.VOXEL, 400_000)
            ctx.scan_prepare(sweeps[0], tt, st, ext, frame.VOXEL, frame.KNN)
            ctx.map_insert_resident(np.eye(4), frame.CAP)
        result["frame"] = measure(dst, src, steps, warmup, frame.CAP)
    vmap = synth.make_map(1_000_000)
    with capi.Context(0) as dst, capi.Context(0) as src:
        for ctx in (dst, src):
            ctx.map_reset(vmap.voxel_size, 2 * vmap.keys.shape[0])          # room for the merged map: no growth inside a timed call
            ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
        result["c2"] = measure(dst, src, max(6, steps // 6), 2, frame.CAP)
    print("PROBE_RESULT " + json.dumps(result), flush=True)


def run_child(steps, warmup, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(steps),
           "--warmup", str(warmup)]
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


def pooled(runs, *path):
    out = []
    for r in runs:
        v = r
        for p in path:
            v = v[p]
        out += v
    return out


def report(name, key, runs):
    r, m = runs[0][key], runs[0][key]["merge"]
    merge_dev, sum_dev = pooled(runs, key, "merge", "dev"), pooled(runs, key, "insert", "sum_dev")
    lines = [f"{name}: {r['voxels']} source voxels into a table of {r['slots']} slots; the merge selects {m['selected']}, creates {m['created']}, "
             f"updates {m['updated']}, freezes out {m['frozen']}, accepts {m['points']} points; {m['launches']} launches",
             f"   vgicp_map_merge, device                               {figure(merge_dev)} us   ({len(merge_dev)} calls)",
             f"   vgicp_map_merge, wall                                 {figure(pooled(runs, key, 'merge', 'wall'))} us",
             f"   from-map + insertion (loses the counts), device       {figure(sum_dev)} us",
             f"      of which vgicp_scan_from_map                       {figure(pooled(runs, key, 'insert', 'sub_dev'))} us",
             f"      of which the insertion (gated at +inf)             {figure(pooled(runs, key, 'insert', 'ins_dev'))} us",
             f"   from-map + insertion, wall of the two calls           {figure(pooled(runs, key, 'insert', 'wall'))} us",
             f"   two vgicp_map_export calls (the counts on the host), wall {figure(pooled(runs, key, 'exports'))} us",
             f"   merge / (from-map + insertion), device medians: {np.median(merge_dev) / np.median(sum_dev):.2f}; the route's p10 - p90 spread "
             f"{np.percentile(sum_dev, 90) - np.percentile(sum_dev, 10):.1f} us, the merge's median minus the route's "
             f"{np.median(merge_dev) - np.median(sum_dev):+.1f} us"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one measuring process may take")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.warmup)
        return
    from eskf_lio_amd import capi
    load0 = os.getloadavg()
    runs = [run_child(a.steps, a.warmup, a.limit) for _ in range(a.processes)]
    load1 = os.getloadavg()
    lines = [f"tools/probe_map_merge.py: {a.processes} processes one after another, {a.steps} timed calls after {a.warmup} per figure and process "
             f"(a sixth on the C2 map), pooled, us, median (p10 - p90)",
             f"one box: {runs[0]['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"library sha256 {frame.sha256(capi.LIB_PATH)}", ""]
    lines += report("1. the second frame's map of bench.py's frame chain, merged into a copy of itself displaced by a frame", "frame", runs) + [""]
    lines += report("2. a C2-size map, likewise", "c2", runs)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
