#!/usr/bin/env python3
"""What the gated map insertion (include/vgicp_hip_map_gated.h) costs beside the plain one.  A developer tool, not a test;
the style of tools/probe_prior.py.

The inputs are the first two frames of bench.py's frame chain: a 60 000-point lidar-like sweep prepared at 0.3 m into an
empty 0.3 m map (vgicp_map_reset with a hint of 400 000, 20 points per voxel), then the second sweep prepared and aligned;
the insertion of that second scan at the aligned pose is what is timed.  Every trial rebuilds this state, so each timed
insertion meets the same map.

  plain         vgicp_map_insert_resident_async with stage events on: vgicp_get_frame_stats' insert_us (the event span
                around the insertion's launches) — on the PARENT's library (--parent) and on the tree's, in alternated
                child processes
  gated async   vgicp_map_insert_resident_gated_async at gate = +inf, the same span (it includes the decision)
  gated         vgicp_map_insert_resident_gated at gate = +inf: vgicp_gated_insert_stats.device_seconds
  report        vgicp_points_resident, counts only, at the same pose before the insertion: device_seconds

    python tools/probe_map_gated.py --parent eskf_lio_amd/lib_ab/parent/libvgicp_hip.so --out profiles/map_gated_timing.txt

Every child runs under its own `timeout -k 10`; the first one that fails ends the run.  A child picks its library through
VGICP_LIB_PATH (eskf_lio_amd/capi.py).
"""
import argparse
import hashlib
import json
import os
import platform
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAP, KNN, VOXEL, POINTS = 20, 30, 0.3, 60_000


def inputs():
    """bench.py frame_chain_leg's world, states and first two sweeps."""
    from eskf_lio_amd import synth
    world = synth.make_lidar_scan(POINTS, seed=0x46524D, extent=25.0)
    st = synth.make_imu_states(48, seed=5)
    st[:, 1:4] = 0.0
    st[:, 4:8] = [0.0, 0.0, 0.0, 1.0]
    tt = synth.make_point_times(POINTS, st[1, 0] + 1e-4, st[-3, 0] + 0.4 / 400.0, seed=5)
    ext = synth.se3_to_SE3([0.01, -0.02, 0.03, 0.002, -0.001, 0.003])
    ext_inv = synth.invert_pose(ext)
    truth = [synth.se3_to_SE3([0.05 * f, 0.02 * f, 0.0, 0.0, 0.0, 0.004 * f]) for f in range(2)]
    rng = np.random.default_rng(12)
    sweeps = []
    for f in range(2):
        Tinv = ext_inv @ synth.invert_pose(truth[f])
        pts = world + rng.normal(scale=0.005, size=world.shape)
        sweeps.append(np.ascontiguousarray(pts @ Tinv[:3, :3].T + Tinv[:3, 3]))
    return sweeps, tt, st, ext


def worker(modes, steps, warmup):
    from eskf_lio_amd import capi
    sweeps, tt, st, ext = inputs()
    result = {"lib": capi.LIB_PATH, "modes": {}}
    with capi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        result["device"] = f"{name}, {cus} compute units"
        ctx.set_option(capi.OPTION_STAGE_EVENTS, 1)
        pose = None

        def rebuild():
            nonlocal pose
            ctx.map_reset(VOXEL, 400_000)
            ctx.scan_prepare(sweeps[0], tt, st, ext, VOXEL, KNN)
            ctx.map_insert_resident(np.eye(4), CAP)
            kept, _ = ctx.scan_prepare(sweeps[1], tt, st, ext, VOXEL, KNN)
            if pose is None:
                pose = ctx.align_resident(np.eye(4), 30, 1e-6, 0.9999).pose
            return kept

        for mode in modes:
            us, extra = [], {}
            for step in range(warmup + steps):
                kept = rebuild()
                voxels = ctx.map_size()[0]
                if mode == "plain":
                    ctx.map_insert_resident_async(pose, CAP)
                    ctx.map_size()
                    t = ctx.frame_stats().insert_us
                elif mode == "gated async":
                    ctx.map_insert_resident_gated_async(pose, CAP, float("inf"))
                    ctx.map_size()
                    t = ctx.frame_stats().insert_us
                    extra = dict(refused=ctx.map_gated_totals()[1])
                elif mode == "gated":
                    _, gs = ctx.map_insert_resident_gated(pose, CAP, float("inf"), kept=False)
                    t = gs.device_seconds * 1e6
                    extra = dict(launches=int(gs.launches), matched=int(gs.matched), refused=int(gs.refused))
                else:
                    rep = ctx.points_resident(pose, (), d2=False, sq_error=False, weight=False, status=False)
                    t = rep.device_seconds * 1e6
                    extra = dict(launches=int(rep.launches), matched=int(rep.matched))
                if step >= warmup:
                    us.append(t)
            d = np.asarray(us)
            result["modes"][mode] = dict(median=float(np.median(d)), p10=float(np.percentile(d, 10)),
                                         p90=float(np.percentile(d, 90)), steps=len(us), points=int(kept),
                                         voxels_before=int(voxels), voxels_after=int(ctx.map_size()[0]), **extra)
    print("PROBE_RESULT " + json.dumps(result), flush=True)


def run_child(lib, modes, steps, warmup, limit):
    env = dict(os.environ, VGICP_LIB_PATH=lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", "--modes", ",".join(modes),
           "--steps", str(steps), "--warmup", str(warmup)]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
        raise SystemExit(f"child ({','.join(modes)} on {lib}) ended with status {proc.returncode}: nothing more is started")
    for line in proc.stdout.splitlines():
        if line.startswith("PROBE_RESULT "):
            return json.loads(line[len("PROBE_RESULT "):])
    raise SystemExit("child printed no result")


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libvgicp_hip.so of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.join(ROOT, "eskf_lio_amd", "lib", "libvgicp_hip.so"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--modes", default="plain")
    a = ap.parse_args()
    if a.worker:
        return worker(tuple(a.modes.split(",")), a.steps, a.warmup)
    if not a.parent:
        raise SystemExit("--parent is required: the baseline is never taken from the tree under test alone")
    parent, tree = os.path.abspath(a.parent), os.path.abspath(a.tree)
    load0 = os.getloadavg()
    series = {"parent": [], "tree": []}
    for _ in range(a.repeats):                                  # alternated: parent, tree, parent, tree ...
        series["parent"].append(run_child(parent, ("plain",), a.steps, a.warmup, a.limit))
        series["tree"].append(run_child(tree, ("plain",), a.steps, a.warmup, a.limit))
    every = run_child(tree, ("plain", "report", "gated async", "gated"), a.steps, a.warmup, a.limit)
    load1 = os.getloadavg()
    first = every["modes"]["plain"]
    lines = [f"tools/probe_map_gated.py: the second frame of bench.py's frame chain ({POINTS}-point sweep -> {first['points']} "
             f"prepared points into a map of {first['voxels_before']} voxels, {CAP} points per voxel), {a.steps} timed insertions "
             f"after {a.warmup} per figure, event-measured device time, us",
             f"one box: {every['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"parent library sha256 {sha256(parent)}", f"tree   library sha256 {sha256(tree)}", "",
             f"1. vgicp_map_insert_resident_async, median per insertion of {a.repeats} alternated child processes each"]
    med = {k: [c["modes"]["plain"]["median"] for c in v] for k, v in series.items()}
    spread = max(med["parent"]) - min(med["parent"])
    lines.append(f"   parent {' '.join('%.2f' % v for v in med['parent'])} (median {np.median(med['parent']):.2f}, spread {spread:.2f})")
    lines.append(f"   tree   {' '.join('%.2f' % v for v in med['tree'])} (median {np.median(med['tree']):.2f})")
    lines += ["", "2. the tree's library, one child: median (p10 - p90)"]
    for mode, r in every["modes"].items():
        rest = {k: v for k, v in r.items() if k not in ("median", "p10", "p90", "steps")}
        lines.append(f"   {mode:12s} {r['median']:8.2f} ({r['p10']:.2f} - {r['p90']:.2f})  {json.dumps(rest)}")
    extra = every["modes"]["gated"]["median"] - float(np.median(med["parent"]))
    lines.append("")
    lines.append(f"the gated call at +inf costs {extra:+.2f} us beside the parent's plain insertion; the counts-only report takes "
                 f"{every['modes']['report']['median']:.2f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
