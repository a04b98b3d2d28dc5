#!/usr/bin/env python3
"""What locate (include/vgicp_hip_map_locate.h) costs, beside what the library offered for the same question before it.
A developer tool, not a test; the pattern of tools/probe_map_levels.py, whose frame-chain state it times on.

Two scenes: the recipe of the locate tests (make_lidar_scan(20000, seed=1) prepared at 0.3 m / 30 neighbours into a 0.3 m
map, cap 1000; the first 6 000 prepared points of the scene at seed 2 resident) and the second frame of bench.py's frame
chain.  Three processes one after the other, each under a time limit of its own; every figure pools their samples:
median (p10 - p90), event-measured device time.

  locate     vgicp_locate_resident on a fan of 64 yaws about a guess (5.1, -3.7, 0.5) m and 37 degrees off, at level 3 with
             the window (4, 4, 1) and at level 2 with (8, 8, 1), strides 1 and 4: vgicp_locate_stats.device_seconds, and the
             call's wall time
  evaluate   what the parent offers: vgicp_evaluate_resident at 64 yaws per call, one call per shifted pose of the
             level-0 window that covers the same metres ((2 * 32 + 1)^2 * (2 * 8 + 1) = 71 825 shifts for both windows).
             A sample of those calls is timed (shifts drawn from the window) and multiplied up: the figure is an
             EXTRAPOLATION from the sample's median, stated as such.

    python tools/probe_map_locate.py --out profiles/map_locate_timing.txt
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

VOXEL = 0.3
SEARCHES = ((3, (4, 4, 1)), (2, (8, 8, 1)))
STRIDES = (1, 4)
YAWS = 64
FINE_WINDOW = (32, 32, 8)          # level-0 voxels that cover 4 x 2.4 m = 8 x 1.2 m, and 1 x 2.4 m
EVAL_SAMPLE = 24                   # evaluate calls timed per process and scene


def wrong_guess():
    a = np.deg2rad(37.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (5.1, -3.7, 0.5)
    return T


def yaw_fan(guess, count):
    out = np.tile(guess, (count, 1, 1))
    for j in range(count):
        a = 2.0 * np.pi * j / count
        out[j, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ guess[:3, :3]
    return out


def measure(ctx, steps, warmup, voxel):
    fan = yaw_fan(wrong_guess(), YAWS)
    out = dict(locate={}, evaluate=[], points=int(ctx.points_size()), voxels=[int(ctx.map_level_size(l)[0]) for l in range(4)],
               slots=[int(ctx.map_level_size(l)[1]) for l in range(4)])
    for level, window in SEARCHES:
        for stride in STRIDES:
            dev, wall, res = [], [], None
            for step in range(warmup + steps):
                res = ctx.locate_resident(fan, level, window, stride, planes=False)
                if res.launches != 2:
                    raise SystemExit(f"a locate made {res.launches} launches")
                if step >= warmup:
                    dev.append(res.device_seconds * 1e6)
                    wall.append(res.seconds * 1e6)
            best = max(res.best, key=lambda b: b["hits"])
            out["locate"][f"{level}/{stride}"] = dict(us=dev, wall=wall, cells=int(res.cells), hits=int(best["hits"]),
                                                      offset=list(best["offset"]))
    rng = np.random.default_rng(1)
    for step in range(2 + EVAL_SAMPLE):
        d = np.array([rng.integers(-w, w + 1) for w in FINE_WINDOW], dtype=np.float64)
        poses = fan.copy()
        poses[:, :3, 3] += d * voxel
        ev = ctx.evaluate_resident(poses)
        if step >= 2:
            out["evaluate"].append([ev.device_seconds * 1e6, ev.seconds * 1e6, int(ev.launches)])
    return out


def worker(steps, warmup):
    from eskf_lio_amd import capi, synth
    result = {}
    with capi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        result["device"] = f"{name}, {cus} compute units"
        ctx.map_reset(VOXEL, 16000)
        ctx.scan_prepare(synth.make_lidar_scan(20000, seed=1), None, None, None, VOXEL, 30)
        ctx.map_insert_resident(np.eye(4), 1000)
        ctx.scan_prepare(synth.make_lidar_scan(20000, seed=2), None, None, None, VOXEL, 30)
        sp, sc = ctx.scan_download()
        ctx.scan_upload(sp[:6000], sc[:6000])
        ctx.map_levels_build(3)
        result["recipe"] = measure(ctx, steps, warmup, VOXEL)
    sweeps, tt, st, ext = frame.inputs()
    with capi.Context(0) as ctx:
        ctx.map_reset(frame.VOXEL, 400_000)
        ctx.scan_prepare(sweeps[0], tt, st, ext, frame.VOXEL, frame.KNN)
        ctx.map_insert_resident(np.eye(4), frame.CAP)
        ctx.scan_prepare(sweeps[1], tt, st, ext, frame.VOXEL, frame.KNN)
        ctx.map_levels_build(3)
        result["frame"] = measure(ctx, steps, warmup, frame.VOXEL)
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
    lines = [f"{name}: {first['points']} resident points; voxels per level {first['voxels']}, slots per level {first['slots']}"]
    ev = [v[0] for r in runs for v in r["evaluate"]]
    ev_wall = [v[1] for r in runs for v in r["evaluate"]]
    shifts = int(np.prod([2 * w + 1 for w in FINE_WINDOW]))
    whole = float(np.median(ev)) * shifts
    lines.append(f"   vgicp_evaluate_resident, {YAWS} poses, one shift              {figure(ev)} us device, {figure(ev_wall)} us wall   "
                 f"({len(ev)} calls, {first['evaluate'][0][2]} launches each)")
    lines.append(f"   ... times the {shifts} shifts of the level-0 window {FINE_WINDOW}: {whole / 1e6:.3f} s of device time, EXTRAPOLATED from that median")
    for level, window in SEARCHES:
        for stride in STRIDES:
            r0 = first["locate"][f"{level}/{stride}"]
            us = [v for r in runs for v in r["locate"][f"{level}/{stride}"]["us"]]
            wall = [v for r in runs for v in r["locate"][f"{level}/{stride}"]["wall"]]
            probes = YAWS * r0["cells"] * -(-first["points"] // stride)
            lines.append(f"   vgicp_locate_resident level {level} window {window} stride {stride}   {figure(us)} us device, {figure(wall)} us wall   "
                         f"({len(us)} calls; {r0['cells']} cells, {probes / 1e6:.1f} M probes = {probes / float(np.median(us)) / 1e3:.1f} G probes/s; "
                         f"best {r0['hits']} hits at {tuple(r0['offset'])}) = the evaluate sweep / {whole / float(np.median(us)):.0f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="seconds one process may take")
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
    lines = [f"tools/probe_map_locate.py: {a.processes} processes one after the other, {a.steps} timed calls after {a.warmup} per figure and "
             f"process ({EVAL_SAMPLE} evaluate calls after 2), event-measured device time, us, median (p10 - p90) over all of them",
             f"one box: {runs[0]['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"library sha256 {frame.sha256(capi.LIB_PATH)}", ""]
    lines += report("1. the recipe of the locate tests", [r["recipe"] for r in runs]) + [""]
    lines += report("2. the second frame of bench.py's frame chain", [r["frame"] for r in runs])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
