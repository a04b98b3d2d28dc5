#!/usr/bin/env python3
"""What free-space carving (include/vgicp_hip_map_carve.h) costs beside the plain insertion.  A developer tool, not a test;
the style of tools/probe_map_gated.py, whose state it times on.

The inputs are the first two frames of bench.py's frame chain: a 60 000-point lidar-like sweep prepared at 0.3 m into an
empty 0.3 m map, then the second sweep prepared and aligned.  Every trial rebuilds this state, so each timed call meets the
same map.

  plain    vgicp_map_insert_resident_async with stage events on: vgicp_get_frame_stats' insert_us (the event span around
           the insertion's launches) — on the PARENT's library (--parent) and on the tree's, in alternated child processes
  carve    vgicp_map_carve_resident at the aligned pose, max_range 20 / 40 / 80 m x stride 1 / 4 (margin one voxel,
           min_hits 2, origin = the extrinsic's translation): vgicp_carve_stats.device_seconds, the event span of the two
           launches; beside it the call's counts, visits per ray, and the mean number of a wave's 64 lanes that are still
           walking per step of the wave's longest ray.  The last is counted on the host, from the numpy restatement of
           the rule (tests/map_carve_reference.py) on the downloaded scan, lane = point index; the restatement's visits are
           checked against the device's first.

    python tools/probe_map_carve.py --parent eskf_lio_amd/lib_ab/parent/libvgicp_hip.so --out profiles/map_carve_timing.txt

Every child runs under its own `timeout -k 10`; the first one that fails ends the run.  A child picks its library through
VGICP_LIB_PATH (eskf_lio_amd/capi.py).
"""
import argparse
import json
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import probe_map_gated as frame  # noqa: E402

RANGES, STRIDES = (20.0, 40.0, 80.0), (1, 4)
MARGIN, MIN_HITS = frame.VOXEL, 2


def lanes_per_step(steps, stride):
    """Mean lanes of a 64-lane wave that are still walking, per step of the wave's longest ray (lane = point index)."""
    n = len(steps)
    padded = np.zeros(-(-n // 64) * 64, dtype=np.int64)
    padded[:n] = np.where(np.arange(n) % stride == 0, steps, 0)
    waves = padded.reshape(-1, 64)
    longest = waves.max(axis=1)
    return float(waves.sum()) / float(max(1, longest.sum()))


def worker(modes, steps, warmup):
    from eskf_lio_amd import capi
    sweeps, tt, st, ext = frame.inputs()
    result = {"lib": capi.LIB_PATH, "modes": {}}
    with capi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        result["device"] = f"{name}, {cus} compute units"
        ctx.set_option(capi.OPTION_STAGE_EVENTS, 1)
        pose = None

        def rebuild():
            nonlocal pose
            ctx.map_reset(frame.VOXEL, 400_000)
            ctx.scan_prepare(sweeps[0], tt, st, ext, frame.VOXEL, frame.KNN)
            ctx.map_insert_resident(np.eye(4), frame.CAP)
            kept, _ = ctx.scan_prepare(sweeps[1], tt, st, ext, frame.VOXEL, frame.KNN)
            if pose is None:
                pose = ctx.align_resident(np.eye(4), 30, 1e-6, 0.9999).pose
            return kept

        for mode in modes:
            us, extra = [], {}
            if mode != "plain":
                import map_carve_reference as mc
                max_range, stride = (float(v) for v in mode.split("/"))
                params = dict(margin=MARGIN, max_range=max_range, min_hits=MIN_HITS, stride=int(stride),
                              origin=tuple(float(v) for v in ext[:3, 3]))
            for step in range(warmup + steps):
                kept = rebuild()
                voxels = ctx.map_size()[0]
                if mode == "plain":
                    ctx.map_insert_resident_async(pose, frame.CAP)
                    ctx.map_size()
                    t = ctx.frame_stats().insert_us
                else:
                    if step == 0:       # the restatement on this very state: its visits must be the device's
                        pts, _ = ctx.scan_download()
                        want = mc.carve(ctx.map_export()[0], frame.VOXEL, pts, pose, mc.Params(**params))
                    _, cs = ctx.map_carve_resident(pose, params, keys=False)
                    t = cs.device_seconds * 1e6
                    got = dict(rays=int(cs.rays), visits=int(cs.visits), touched=int(cs.touched), shielded=int(cs.shielded),
                               removed=int(cs.removed))
                    if got != want.counts():
                        raise SystemExit(f"{mode}: the device's counts {got} are not the restatement's {want.counts()}")
                    extra = dict(got, launches=int(cs.launches), visits_per_ray=round(cs.visits / max(1, cs.rays), 1),
                                 lanes_per_step=round(lanes_per_step(want.steps, int(stride)), 1))
                if step >= warmup:
                    us.append(t)
            d = np.asarray(us)
            result["modes"][mode] = dict(median=float(np.median(d)), p10=float(np.percentile(d, 10)),
                                         p90=float(np.percentile(d, 90)), steps=len(us), points=int(kept),
                                         voxels_before=int(voxels), **extra)
    print("PROBE_RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libvgicp_hip.so of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.join(ROOT, "eskf_lio_amd", "lib", "libvgicp_hip.so"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds a child may take")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--modes", default="plain")
    a = ap.parse_args()
    if a.worker:
        return worker(tuple(a.modes.split(",")), a.steps, a.warmup)
    if not a.parent:
        raise SystemExit("--parent is required: the baseline is never taken from the tree under test alone")
    parent, tree = os.path.abspath(a.parent), os.path.abspath(a.tree)
    frame.__file__ = os.path.abspath(__file__)        # run_child starts THIS file's worker
    load0 = os.getloadavg()
    series = {"parent": [], "tree": []}
    for _ in range(a.repeats):                                  # alternated: parent, tree, parent, tree ...
        series["parent"].append(frame.run_child(parent, ("plain",), a.steps, a.warmup, a.limit))
        series["tree"].append(frame.run_child(tree, ("plain",), a.steps, a.warmup, a.limit))
    carve_modes = tuple(f"{r:g}/{s}" for r in RANGES for s in STRIDES)
    every = frame.run_child(tree, carve_modes, a.steps, a.warmup, a.limit)
    load1 = os.getloadavg()
    first = series["tree"][0]["modes"]["plain"]
    lines = [f"tools/probe_map_carve.py: the second frame of bench.py's frame chain ({frame.POINTS}-point sweep -> {first['points']} "
             f"prepared points, a map of {first['voxels_before']} voxels of {frame.VOXEL} m), {a.steps} timed calls after {a.warmup} "
             f"per figure, event-measured device time, us",
             f"one box: {every['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"parent library sha256 {frame.sha256(parent)}", f"tree   library sha256 {frame.sha256(tree)}", "",
             f"1. vgicp_map_insert_resident_async, median per insertion of {a.repeats} alternated child processes each"]
    med = {k: [c["modes"]["plain"]["median"] for c in v] for k, v in series.items()}
    spread = max(med["parent"]) - min(med["parent"])
    lines.append(f"   parent {' '.join('%.2f' % v for v in med['parent'])} (median {np.median(med['parent']):.2f}, spread {spread:.2f})")
    lines.append(f"   tree   {' '.join('%.2f' % v for v in med['tree'])} (median {np.median(med['tree']):.2f})")
    lines += ["", f"2. vgicp_map_carve_resident (margin {MARGIN} m, min_hits {MIN_HITS}), the tree's library, one child: the two launches' "
                  "event span, median (p10 - p90)",
              "   max_range/stride      us                     rays    visits  visits/ray  lanes/step  touched shielded  removed"]
    for mode, r in every["modes"].items():
        lines.append(f"   {mode:>8s}       {r['median']:8.2f} ({r['p10']:7.2f} - {r['p90']:7.2f})  {r['rays']:7d} {r['visits']:9d}  {r['visits_per_ray']:9.1f}"
                     f"  {r['lanes_per_step']:10.1f}  {r['touched']:7d}  {r['shielded']:7d}  {r['removed']:7d}")
    lines += ["", "lanes/step: of a wave's 64 lanes, how many are still walking per step of its longest ray (host count on the "
                  "numpy restatement, whose counts equal the device's)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
