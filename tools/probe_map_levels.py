#!/usr/bin/env python3
"""What the map's coarser levels (include/vgicp_hip_map_levels.h) cost beside the work a frame does anyway.  A developer
tool, not a test; the pattern of tools/probe_map_rays.py, whose frame-chain state it times on.

Two maps: the second frame of bench.py's frame chain (a 60 000-point lidar-like sweep prepared at 0.3 m into an empty map
made with bench.py's capacity hint, then the second sweep prepared and aligned), and a C2-size map (1 M voxels mirrored
with vgicp_map_upsert, a 100 000-point uniform scan resident).  Three processes one after the other, each under a time
limit of its own; every figure pools their samples: median (p10 - p90), event-measured device time.

  build    vgicp_map_levels_build(L), L = 1, 2, 3, each time after a map change that changes no voxel (an erase of a key the
           map does not hold moves the map's version): vgicp_levels_stats.device_seconds and .launches.  The levels'
           storage exists already, as in every frame but the first.
  insert   the plain vgicp_map_insert_resident_async of the same scan into the same map, settled: the frame statistics'
           insert_us (VGICP_OPTION_STAGE_EVENTS), the map made anew in front of every call
  align    vgicp_align_resident_levels 3 -> 2 -> 1 -> 0 from the frame's guess (coarse stages 30 / 1e-4 / 0.999, the fine
           stage 100 / 1e-6 / 0.9999): vgicp_stats.device_seconds of every stage, beside vgicp_align_resident with the
           fine stage's thresholds from the same guess

    python tools/probe_map_levels.py --out profiles/map_levels_timing.txt
"""
import argparse
import json
import os
import platform
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import probe_map_gated as frame  # noqa: E402

COARSE = dict(max_iteration=30, translation_sq_threshold=1e-4, cosine_threshold=0.999)
FINE = dict(max_iteration=100, translation_sq_threshold=1e-6, cosine_threshold=0.9999)
SCHEDULE = (3, 2, 1, 0)
ABSENT_KEY = np.array([[1 << 29, 1 << 29, 1 << 29]], dtype=np.int32)
C2_POINTS, C2_VOXELS = 100_000, 1_000_000


def measure(ctx, capi, steps, warmup, remake, guess, cap):
    """The three measurements on a context whose map and resident scan `remake()` puts into their state."""
    out = dict(build={}, align=[], plain_align=[], insert=[])
    remake()
    for levels in (1, 2, 3):
        ctx.map_levels_build(levels)                # storage
        us, st = [], None
        for step in range(warmup + steps):
            ctx.map_erase(ABSENT_KEY)               # the map's version moves, no voxel does
            st = ctx.map_levels_build(levels)
            if st.launches != 2 * levels:
                raise SystemExit(f"a rebuild of {levels} levels made {st.launches} launches")
            if step >= warmup:
                us.append(st.device_seconds * 1e6)
        out["build"][levels] = dict(us=us, launches=int(st.launches), voxels=list(st.voxels), slots=list(st.slots))
    for step in range(warmup + steps):
        _, stages = ctx.align_resident_levels(guess, SCHEDULE, [COARSE] * 3 + [FINE], allow_degenerate=True)
        plain = ctx.align_resident(guess, FINE["max_iteration"], FINE["translation_sq_threshold"], FINE["cosine_threshold"],
                                   allow_degenerate=True)
        if step >= warmup:
            out["align"].append([[s.device_seconds * 1e6, int(s.iterations), int(s.launches)] for s in stages])
            out["plain_align"].append([plain.device_seconds * 1e6, int(plain.iterations), int(plain.launches)])
    ctx.map_levels_build(0)                         # the insertion is the parent's: a context without levels
    for step in range(min(warmup, 1) + max(3, steps // 3)):
        pose = remake()
        ctx.map_insert_resident_async(pose, cap)
        ctx.map_size()
        if step >= min(warmup, 1):
            out["insert"].append(ctx.frame_stats().insert_us)
    return out


def worker(steps, warmup):
    from eskf_lio_amd import capi, synth
    sweeps, tt, st, ext = frame.inputs()
    result = {}
    with capi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        result["device"] = f"{name}, {cus} compute units"
        ctx.set_option(capi.OPTION_STAGE_EVENTS, 1)
        state = dict(pose=None, kept=0)

        def remake_frame():
            ctx.map_reset(frame.VOXEL, 400_000)
            ctx.scan_prepare(sweeps[0], tt, st, ext, frame.VOXEL, frame.KNN)
            ctx.map_insert_resident(np.eye(4), frame.CAP)
            state["kept"], _ = ctx.scan_prepare(sweeps[1], tt, st, ext, frame.VOXEL, frame.KNN)
            if state["pose"] is None:
                state["pose"] = ctx.align_resident(np.eye(4), 30, 1e-6, 0.9999).pose
            return state["pose"]

        result["frame"] = measure(ctx, capi, steps, warmup, remake_frame, np.eye(4), frame.CAP)
        result["frame"]["points"] = int(state["kept"])
    vmap = synth.make_map(C2_VOXELS)
    pts, covs = synth.make_uniform_scan(C2_POINTS, vmap)
    guess = synth.default_guess()
    with capi.Context(0) as ctx:
        ctx.set_option(capi.OPTION_STAGE_EVENTS, 1)

        def remake_c2():
            ctx.map_reset(vmap.voxel_size, C2_VOXELS)
            ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
            ctx.scan_upload(pts, covs)
            return guess

        result["c2"] = measure(ctx, capi, max(3, steps // 2), min(warmup, 2), remake_c2, guess, frame.CAP)
        result["c2"]["points"] = C2_POINTS
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
    return f"{np.median(d):9.2f} ({np.percentile(d, 10):9.2f} - {np.percentile(d, 90):9.2f})"


def report(name, runs):
    first = runs[0]
    b3 = first["build"]["3"]
    lines = [f"{name}: {first['points']} resident points; voxels per level {b3['voxels'][:4]}, slots per level {b3['slots'][:4]}"]
    insert = [v for r in runs for v in r["insert"]]
    lines.append(f"   plain vgicp_map_insert_resident_async                  {figure(insert)} us   ({len(insert)} calls)")
    for levels in ("1", "2", "3"):
        us = [v for r in runs for v in r["build"][levels]["us"]]
        ratio = float(np.median(us)) / float(np.median(insert))
        lines.append(f"   vgicp_map_levels_build({levels}), {first['build'][levels]['launches']} launches                    {figure(us)} us   "
                     f"({len(us)} calls) = {ratio:.2f} x the insertion")
    plain = [v[0] for r in runs for v in r["plain_align"]]
    p0 = first["plain_align"][0]
    lines.append(f"   plain vgicp_align_resident                             {figure(plain)} us   ({p0[1]} rounds, {p0[2]} launch(es))")
    total = [sum(s[0] for s in a) for r in runs for a in r["align"]]
    for i, level in enumerate(SCHEDULE):
        us = [a[i][0] for r in runs for a in r["align"]]
        s0 = first["align"][0][i]
        lines.append(f"   stage {i}, level {level}                                       {figure(us)} us   ({s0[1]} rounds, {s0[2]} launch(es))")
    lines.append(f"   the four stages together                               {figure(total)} us = "
                 f"{float(np.median(total)) / float(np.median(plain)):.2f} x the plain align")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one process may take")
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
    lines = [f"tools/probe_map_levels.py: {a.processes} processes one after the other, {a.steps} timed calls after {a.warmup} per figure and "
             "process (C2 and the insertions: fewer, see the counts), event-measured device time, us, median (p10 - p90) over all of them",
             f"one box: {runs[0]['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"library sha256 {frame.sha256(capi.LIB_PATH)}", ""]
    lines += report("1. the second frame of bench.py's frame chain", [r["frame"] for r in runs]) + [""]
    lines += report("2. a C2-size map", [r["c2"] for r in runs])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
