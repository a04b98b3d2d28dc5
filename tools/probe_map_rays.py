#!/usr/bin/env python3
"""What the ray report (include/vgicp_hip_map_rays.h) costs beside free-space carving.  A developer tool, not a test; the
pattern of tools/probe_map_carve.py, whose state it times on.

The inputs are the first two frames of bench.py's frame chain: a 60 000-point lidar-like sweep prepared at 0.3 m into an
empty 0.3 m map, then the second sweep prepared and aligned.  One process, two contexts in the same state:

  report   vgicp_rays_resident at the aligned pose, max_range 20 / 40 m x stride 1 / 4 x beyond 0 / 20 m (margin one voxel,
           origin = the extrinsic's translation), counts only: vgicp_ray_stats.device_seconds, the event span around the
           bitmap clear and the two launches.  Read-only, so every call meets the same map.  Its counts are checked
           against the numpy restatement (tests/map_rays_reference.py) first.
  floor    the same call with a stride beyond the scan's size: one ray; the clear, CONFIRM and an all but empty WALK
  carve    vgicp_map_carve_resident at the same range, stride and margin (min_hits 2) on a COPY of the map: a second
           context that is rebuilt by the same two frames in front of every call: vgicp_carve_stats.device_seconds
  poses    vgicp_rays_resident at 16 and 64 poses around the aligned one (max_range 40 m, stride 1, beyond 0): poses per
           second by the call's device time and by its wall time

    python tools/probe_map_rays.py --out profiles/map_rays_timing.txt
"""
import argparse
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import probe_map_gated as frame  # noqa: E402

RANGES, STRIDES, BEYONDS = (20.0, 40.0), (1, 4), (0.0, 20.0)
MARGIN, MIN_HITS = frame.VOXEL, 2


def summary(us):
    d = np.asarray(us)
    return float(np.median(d)), float(np.percentile(d, 10)), float(np.percentile(d, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    from eskf_lio_amd import capi
    import map_rays_reference as mr
    sweeps, tt, st, ext = frame.inputs()
    origin = tuple(float(v) for v in ext[:3, 3])
    load0 = os.getloadavg()
    with capi.Context(0) as ctx, capi.Context(0) as copy:
        name, cus, _ = ctx.device_info()
        pose = None

        def rebuild(c):
            nonlocal pose
            c.map_reset(frame.VOXEL, 400_000)
            c.scan_prepare(sweeps[0], tt, st, ext, frame.VOXEL, frame.KNN)
            c.map_insert_resident(np.eye(4), frame.CAP)
            kept, _ = c.scan_prepare(sweeps[1], tt, st, ext, frame.VOXEL, frame.KNN)
            if pose is None:
                pose = c.align_resident(np.eye(4), 30, 1e-6, 0.9999).pose
            return kept

        kept = rebuild(ctx)
        voxels, slots = ctx.map_size()
        pts, _ = ctx.scan_download()
        map_keys = ctx.map_export()[0]
        rows = []
        for max_range in RANGES:
            for stride in STRIDES:
                carve = dict(margin=MARGIN, max_range=max_range, min_hits=MIN_HITS, stride=stride, origin=origin)
                us, cs = [], None
                for step in range(a.warmup + a.steps):
                    rebuild(copy)
                    _, cs = copy.map_carve_resident(pose, carve, keys=False)
                    if step >= a.warmup:
                        us.append(cs.device_seconds * 1e6)
                row = dict(max_range=max_range, stride=stride, carve=summary(us), carve_rays=int(cs.rays), carve_visits=int(cs.visits),
                           report={})
                for beyond in BEYONDS:
                    params = dict(margin=MARGIN, beyond=beyond, max_range=max_range, stride=stride, origin=origin)
                    want = mr.rays(map_keys, frame.VOXEL, pts, pose, mr.Params(**params)).counts()
                    us, rep = [], None
                    for step in range(a.warmup + a.steps):
                        rep = ctx.rays_resident(pose, params, per_point=False)
                        if step >= a.warmup:
                            us.append(rep.device_seconds * 1e6)
                    if rep.counts[0] != want:
                        raise SystemExit(f"{max_range}/{stride}/{beyond}: the device's counts {rep.counts[0]} are not the restatement's {want}")
                    row["report"][beyond] = dict(us=summary(us), **rep.counts[0])
                rows.append(row)
        # the floor: one ray
        us = []
        for step in range(a.warmup + a.steps):
            rep = ctx.rays_resident(pose, dict(margin=MARGIN, beyond=0.0, max_range=40.0, stride=int(kept) + 1, origin=origin), per_point=False)
            if step >= a.warmup:
                us.append(rep.device_seconds * 1e6)
        floor = summary(us)
        # several poses
        many = []
        for k in (16, 64):
            poses = []
            for f in range(k):
                P = np.array(pose)
                P[:3, 3] += (0.02 * f, -0.01 * f, 0.0)
                poses.append(P)
            dev, wall = [], []
            for step in range(a.warmup + 10):
                rep = ctx.rays_resident(poses, dict(margin=MARGIN, beyond=0.0, max_range=40.0, stride=1, origin=origin))
                if step >= a.warmup:
                    dev.append(rep.device_seconds)
                    wall.append(rep.seconds)
            many.append((k, rep.groups, rep.launches, float(np.median(dev)), float(np.median(wall))))
    load1 = os.getloadavg()

    lines = [f"tools/probe_map_rays.py: the second frame of bench.py's frame chain ({frame.POINTS}-point sweep -> {kept} prepared points, a map "
             f"of {voxels} voxels of {frame.VOXEL} m in {slots} slots), {a.steps} timed calls after {a.warmup} per figure, event-measured device "
             "time, us, median (p10 - p90); one process",
             f"one box: {name}, {cus} compute units, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"library sha256 {frame.sha256(capi.LIB_PATH)}", "",
             f"1. vgicp_rays_resident (margin {MARGIN} m, counts only) beside vgicp_map_carve_resident (margin {MARGIN} m, min_hits {MIN_HITS}) on a "
             "copy of the map, same max_range and stride",
             "   max_range/stride   carve us                   visits    report, beyond 0 us          visits    report, beyond 20 us         visits"]
    notes = []
    for r in rows:
        c, r0, r20 = r["carve"], r["report"][0.0], r["report"][20.0]
        lines.append(f"   {r['max_range']:>5g}/{r['stride']}        {c[0]:8.2f} ({c[1]:7.2f} - {c[2]:7.2f}) {r['carve_visits']:9d}   "
                     f"{r0['us'][0]:8.2f} ({r0['us'][1]:7.2f} - {r0['us'][2]:7.2f}) {r0['visits']:9d}   "
                     f"{r20['us'][0]:8.2f} ({r20['us'][1]:7.2f} - {r20['us'][2]:7.2f}) {r20['visits']:9d}")
        over, spread = r0["us"][0] - c[0], c[2] - c[1]
        verdict = "within" if over <= spread else "ABOVE"
        notes.append(f"   {r['max_range']:g}/{r['stride']}: report - carve = {over:+.2f} us, carve's p10 - p90 spread {spread:.2f} us: {verdict} it; "
                     f"visits {r0['visits']} against {r['carve_visits']} ({r0['visits'] / max(1, r['carve_visits']):.2f} x), rays {r0['rays']} / {r['carve_rays']}")
    lines += ["", "2. the report's median at beyond 0 against carve's, in carve's own spread of this run"] + notes
    lines += [f"   the floor, one ray (stride {kept + 1}): {floor[0]:.2f} us ({floor[1]:.2f} - {floor[2]:.2f}): the clear of the {slots // 8}-byte "
              "bitmap, CONFIRM over every point and an all but empty WALK",
              "   where the report is ABOVE: it pays the floor's bitmap clear and CONFIRM launch in front of its walks, which carve's mark "
              "launch folds into one kernel; where it is below: its walks end at the first FULL voxel (the visits above) and probe "
              "without an atomic add per FULL voxel, while carve walks every ray to its end and sweeps the slots afterwards",
              "", "3. classes at max_range 40, stride 1 (no_ray open own behind confirmed blocked near):"]
    for beyond in BEYONDS:
        r = next(x for x in rows if x["max_range"] == 40.0 and x["stride"] == 1)["report"][beyond]
        lines.append(f"   beyond {beyond:g}: {' '.join(str(v) for v in r['by_class'][:7])}")
    lines += ["", "4. several poses in one call (max_range 40, stride 1, beyond 0)"]
    for k, groups, launches, dev, wall in many:
        lines.append(f"   {k:2d} poses: {groups} group(s), {launches} launches, device {1e6 * dev:9.2f} us = {k / dev:9.0f} poses/s, "
                     f"wall {1e6 * wall:9.2f} us = {k / wall:9.0f} poses/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
