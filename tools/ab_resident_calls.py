#!/usr/bin/env python3
"""The four calls over the resident scan at a pose on two builds of the library: host wall time and event-measured device
time of vgicp_evaluate_resident, vgicp_align_resident_batch, vgicp_points_resident and vgicp_map_insert_resident_gated as
each call's own stats report them.  A developer tool, not a test; the workloads are those of tools/ab_evaluate.py,
tools/ab_align_batch.py and tools/probe_map_gated.py.

  evaluate   synth.make_map(50_000), synth.make_structured_scan(27_000) resident, ONE call with k = 16 poses
  batch      the same scene, ONE call with k = 4 guesses, 20 forced rounds
  report     the second frame of bench.py's frame chain (tools/probe_map_gated.py's state: a 60 000-point sweep prepared
             at 0.3 m, aligned): counts and five quantiles, no per-point array
  gated      that scan inserted at the aligned pose with gate = +inf, kept not asked; the state is rebuilt for every call

The baseline is ANOTHER build (--parent), never the tree under test alone; the two are timed in alternated child
processes (parent, tree, tree, parent, ...: neither build always follows the other), each under its own `timeout -k 10`;
the first child that fails ends the run.  A repetition is one child: the median over its calls.  Reported per call: each
build's median over its repetitions and the parent's own min .. max, inside which the tree's median should lie when only
host instructions changed.

    python tools/ab_resident_calls.py --parent eskf_lio_amd/lib_ab/parent/libvgicp_hip.so --out profiles/resident_calls_timing.txt
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
CALLS = ("evaluate", "batch", "report", "gated")
QS = (0.1, 0.25, 0.5, 0.75, 0.9)


def worker(steps, warmup):
    from eskf_lio_amd import capi, synth
    import probe_map_gated as frame
    out = {"lib": capi.LIB_PATH, "calls": {}}

    def timed(name, call, n, before=lambda: None):
        wall, dev = [], []
        for step in range(warmup + n):
            before()
            st = call()
            if step >= warmup:
                wall.append(st.seconds * 1e6)
                dev.append(st.device_seconds * 1e6)
        out["calls"][name] = dict(wall=float(np.median(wall)), device=float(np.median(dev)), launches=int(st.launches), steps=n)

    with capi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        out["device"] = f"{name}, {cus} compute units"
        vmap = synth.make_map(50_000)
        pts, covs, T_true = synth.make_structured_scan(27_000, vmap)
        ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0])
        ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
        ctx.scan_upload(pts, covs)
        rng = np.random.default_rng(5)
        poses = [synth.se3_to_SE3(np.asarray(synth.GUESS_XI) + 0.01 * rng.standard_normal(6)) for _ in range(16)]
        timed("evaluate", lambda: ctx.evaluate_resident(poses), steps)
        timed("batch", lambda: ctx.align_resident_batch(poses[:4], 20, 1e-6, 2.0), steps // 2)
    with capi.Context(0) as ctx:
        sweeps, tt, st, ext = frame.inputs()
        state = {}

        def rebuild():
            ctx.map_reset(frame.VOXEL, 400_000)
            ctx.scan_prepare(sweeps[0], tt, st, ext, frame.VOXEL, frame.KNN)
            ctx.map_insert_resident(np.eye(4), frame.CAP)
            ctx.scan_prepare(sweeps[1], tt, st, ext, frame.VOXEL, frame.KNN)
            if "pose" not in state:
                state["pose"] = ctx.align_resident(np.eye(4), 30, 1e-6, 0.9999).pose

        rebuild()
        timed("report", lambda: ctx.points_resident(state["pose"], QS, d2=False, sq_error=False, weight=False, status=False), steps)
        timed("gated", lambda: ctx.map_insert_resident_gated(state["pose"], frame.CAP, float("inf"), kept=False)[1],
              max(steps // 4, 5), before=rebuild)
    print("AB_RESULT " + json.dumps(out), flush=True)


def run_child(lib, steps, warmup, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(steps),
           "--warmup", str(warmup)]
    proc = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, VGICP_LIB_PATH=lib), capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
        raise SystemExit(f"child on {lib} ended with status {proc.returncode}: nothing more is started")
    for line in proc.stdout.splitlines():
        if line.startswith("AB_RESULT "):
            return json.loads(line[len("AB_RESULT "):])
    raise SystemExit("child printed no result")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libvgicp_hip.so of the parent commit (the baseline), its side libraries beside it")
    ap.add_argument("--tree", default=os.path.join(ROOT, "eskf_lio_amd", "lib", "libvgicp_hip.so"))
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.steps, a.warmup)
    if not a.parent:
        raise SystemExit("--parent is required: the baseline is never taken from the tree under test alone")
    libs = {"parent": os.path.abspath(a.parent), "tree": os.path.abspath(a.tree)}
    load0 = os.getloadavg()
    runs = {"parent": [], "tree": []}
    for rep in range(a.repeats):                                # alternated: parent, tree, tree, parent, parent ...
        for build in (("parent", "tree") if rep % 2 == 0 else ("tree", "parent")):
            runs[build].append(run_child(libs[build], a.steps, a.warmup, a.limit))
    first = runs["tree"][0]
    lines = ["the calls over the resident scan at a pose, parent build against tree build (tools/ab_resident_calls.py)",
             f"device: {first['device']}; host: {platform.node()}; load average {load0[0]:.1f} -> {os.getloadavg()[0]:.1f}",
             *(f"{b}: {libs[b]} sha256 {hashlib.sha256(open(libs[b], 'rb').read()).hexdigest()[:16]}" for b in libs),
             f"{a.repeats} alternated child processes per build; a repetition is the median over a child's calls (us)", ""]
    inside = True
    for call in CALLS:
        c = first["calls"][call]
        lines.append(f"{call}: {c['steps']} calls per repetition, {c['launches']} launches per call")
        for what in ("wall", "device"):
            p = np.asarray([r["calls"][call][what] for r in runs["parent"]])
            t = np.asarray([r["calls"][call][what] for r in runs["tree"]])
            ok = p.min() <= np.median(t) <= p.max()
            inside = inside and ok
            lines.append(f"  {what:6s} parent median {np.median(p):9.2f} ({p.min():9.2f} .. {p.max():9.2f})   tree median "
                         f"{np.median(t):9.2f} ({t.min():9.2f} .. {t.max():9.2f})   {'inside' if ok else 'OUTSIDE'} the parent's spread")
            lines.append(f"         parent {' '.join('%.2f' % v for v in p)}")
            lines.append(f"         tree   {' '.join('%.2f' % v for v in t)}")
    lines.append("")
    lines.append("every tree median lies inside the parent's own min .. max" if inside else
                 "NOT every tree median lies inside the parent's own min .. max")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
