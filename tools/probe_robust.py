#!/usr/bin/env python3
"""What the robust rounds (include/vgicp_hip_robust.h) cost, and that the plain path does not pay for them.  A developer
tool, not a test.

The workload is bench.py's C2, resident: synth.make_map(1_000_000), synth.make_uniform_scan(100_000), 20 forced rounds
(translation_sq_threshold 1e-6, cosine_threshold 2.0), >= 200 timed vgicp_align_resident calls per figure after warm-up.

1. The plain path, mode off, on the PARENT's library (--parent, never the tree under test alone) and on the tree's, in
   alternated child processes (parent, tree, parent, tree ...), five of each by default: the median event-measured
   device_seconds per align of every child.  Accepted when the two medians differ by no more than the spread (max - min)
   of the parent's own repetitions.
2. Every mode on the tree's library in one child: plain, Cauchy 0.15 + gate 0.06 and Huber 0.08, each on the persistent
   launch and on the launch-per-round loop (VGICP_FLAG_NO_PERSISTENT): device time per round, give-ups.
3. --trace: two more children of the tree's library under `rocprofv3 --kernel-trace --stats`, runs of their own — one
   with Cauchy + gate, one with Huber as the robust mode, each beside the plain persistent launch and the plain loop of
   the same run — and the kernels' own times per round from the statistics.  Sanity condition: the robust persistent
   round must be faster than the plain launch-per-round loop of the same run.

    python tools/probe_robust.py --parent eskf_lio_amd/lib_ab/parent/libvgicp_hip.so --trace --out profiles/r24_robust.txt

Every child runs under its own `timeout -k 10`; the first one that fails ends the run.  A child picks its library
through VGICP_LIB_PATH (eskf_lio_amd/capi.py).
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import platform
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 20
MODES = {"plain": ("none", 1.0, 0.0), "cauchy+gate": ("cauchy", 0.15, 0.06), "huber": ("huber", 0.08, 0.0)}


def worker(modes, steps, warmup):
    from eskf_lio_amd import capi, synth
    vmap = synth.make_map(1_000_000)
    pts, covs = synth.make_uniform_scan(100_000, vmap)
    guess = synth.default_guess()
    result = {"lib": capi.LIB_PATH, "modes": {}}
    with capi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        result["device"] = f"{name}, {cus} compute units"
        ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0])
        ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)
        ctx.scan_upload(pts, covs)
        for mode in modes:
            if mode != "plain":                                  # the parent's library has no such option: never set there
                ctx.set_robust(*MODES[mode])
            for path, flags in (("persistent", 0), ("loop", capi.FLAG_NO_PERSISTENT)):
                dev, counts = [], None
                for step in range(warmup + steps):
                    r = ctx.align_resident(guess, ROUNDS, 1e-6, 2.0, flags=flags)
                    if step >= warmup:
                        dev.append(r.device_seconds * 1e6)
                    counts = r.corr_count
                d = np.asarray(dev)
                result["modes"][f"{mode}/{path}"] = dict(
                    median=float(np.median(d)), p10=float(np.percentile(d, 10)), p90=float(np.percentile(d, 90)),
                    steps=len(dev), launches=int(r.launches), rounds=int(r.iterations),
                    count_first=int(counts[0]), count_last=int(counts[-1]))
            if mode != "plain":
                ctx.set_robust("none", 1.0, 0.0)
        result["fallbacks"] = ctx.counter(1)
    print("PROBE_RESULT " + json.dumps(result), flush=True)


def child_command(modes, steps, warmup):
    return [sys.executable, os.path.abspath(__file__), "--worker", "--modes", ",".join(modes), "--steps", str(steps),
            "--warmup", str(warmup)]


def run_child(lib, modes, steps, warmup, limit):
    env = dict(os.environ, VGICP_LIB_PATH=lib)
    proc = subprocess.run(["timeout", "-k", "10", str(limit)] + child_command(modes, steps, warmup), cwd=ROOT, env=env,
                          capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
        raise SystemExit(f"child ({','.join(modes)} on {lib}) ended with status {proc.returncode}: nothing more is started")
    for line in proc.stdout.splitlines():
        if line.startswith("PROBE_RESULT "):
            return json.loads(line[len("PROBE_RESULT "):])
    raise SystemExit("child printed no result")


def kernel_trace(tree, robust_mode, steps, warmup, limit):
    """One child (plain and `robust_mode`, both paths) under rocprofv3 --kernel-trace --stats -> report lines."""
    calls = warmup + steps
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, VGICP_LIB_PATH=tree)
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
               "--"] + child_command(("plain", robust_mode), steps, warmup)
        proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
        if proc.returncode != 0:
            sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
            raise SystemExit(f"the traced child ended with status {proc.returncode}")
        rows = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "").replace("(bool)", "")
                no, yes = "(?:false|0)", "(?:true|1)"
                for short, pattern in (("persistent, plain", f"persistent_kernel<512, {no}, {no}, {no}, {no}>"),
                                       ("persistent, robust", f"persistent_kernel<512, {no}, {no}, {no}, {yes}>"),
                                       ("loop round, plain", f"iterate_kernel<512, {no}>"),
                                       ("loop round, robust", f"iterate_kernel<512, {yes}>")):
                    if re.search(pattern, name):
                        rows[short] = (int(row["Calls"]), int(row["Calls"]) * float(row["AverageNs"]) / 1e3)
    lines = [f"rocprofv3 --kernel-trace --stats, a run of its own: plain and {robust_mode} "
             f"({MODES[robust_mode][0]} {MODES[robust_mode][1]}, gate {MODES[robust_mode][2]}), {calls} aligns of {ROUNDS} rounds per "
             f"mode and path"]
    per_round = {}
    for short in ("persistent, plain", "persistent, robust", "loop round, plain", "loop round, robust"):
        if short not in rows:
            lines.append(f"  {short:20s} (not in the profiler's statistics)")
            continue
        n, total = rows[short]
        rounds = n * ROUNDS if short.startswith("persistent") else n
        per_round[short] = total / rounds
        lines.append(f"  {short:20s} calls {n:6d}  total {total / 1e3:9.2f} ms  {per_round[short]:6.2f} us per round")
    if "persistent, robust" in per_round and "loop round, plain" in per_round:
        ok = per_round["persistent, robust"] < per_round["loop round, plain"]
        lines.append(f"  sanity: the robust persistent round ({per_round['persistent, robust']:.2f} us) is "
                     f"{'faster' if ok else 'NOT faster'} than the plain launch-per-round loop's kernel alone "
                     f"({per_round['loop round, plain']:.2f} us, launch gaps not counted)")
    return lines


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libvgicp_hip.so of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.join(ROOT, "eskf_lio_amd", "lib", "libvgicp_hip.so"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--limit", type=int, default=150, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true", help="also two children under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--modes", default="plain")
    a = ap.parse_args()
    if a.worker:
        return worker(tuple(a.modes.split(",")), a.steps, a.warmup)
    if not a.parent:
        raise SystemExit("--parent is required: the baseline is never taken from the tree under test alone")
    if a.steps < 200:
        raise SystemExit("--steps must be at least 200")
    parent, tree = os.path.abspath(a.parent), os.path.abspath(a.tree)
    load0 = os.getloadavg()
    series = {"parent": [], "tree": []}
    for _ in range(a.repeats):                                  # alternated: parent, tree, parent, tree ...
        series["parent"].append(run_child(parent, ("plain",), a.steps, a.warmup, a.limit))
        series["tree"].append(run_child(tree, ("plain",), a.steps, a.warmup, a.limit))
    every = run_child(tree, tuple(MODES), a.steps, a.warmup, a.limit)
    load1 = os.getloadavg()
    lines = [f"tools/probe_robust.py: C2 resident (100 000-point uniform scan, 1 000 000 voxels, {ROUNDS} forced rounds), {a.steps} "
             f"timed aligns after {a.warmup} per figure, event-measured device time, us",
             f"one box: {every['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"parent library sha256 {sha256(parent)}", f"tree   library sha256 {sha256(tree)}", "",
             f"1. the plain path, mode off: median device time per align of {a.repeats} alternated child processes each"]
    verdicts = []
    for path in ("persistent", "loop"):
        p = [r["modes"][f"plain/{path}"]["median"] for r in series["parent"]]
        t = [r["modes"][f"plain/{path}"]["median"] for r in series["tree"]]
        spread, delta = max(p) - min(p), float(np.median(t) - np.median(p))
        ok = abs(delta) <= spread
        verdicts.append(ok)
        lines += [f"  {path:10s} parent " + " ".join(f"{v:8.2f}" for v in p) + f"   median {np.median(p):8.2f}  spread {spread:.2f}",
                  f"  {path:10s} tree   " + " ".join(f"{v:8.2f}" for v in t) + f"   median {np.median(t):8.2f}  "
                  f"difference {delta:+.2f} ({100 * delta / np.median(p):+.2f} %): "
                  f"{'within' if ok else 'BEYOND'} the parent's own spread"]
    lines += ["", "2. every mode on the tree's library, one child: device time per align / per round, counts of the first and last round"]
    for key, m in every["modes"].items():
        lines.append(f"  {key:24s} {m['median']:8.2f} us per align (p10 {m['p10']:.2f}, p90 {m['p90']:.2f})  {m['median'] / m['rounds']:6.2f} us "
                     f"per round  launches {m['launches']:2d}  counts {m['count_first']} -> {m['count_last']}")
    lines.append(f"  persistent launches that gave up: {every['fallbacks']}")
    rp, pl = every["modes"]["cauchy+gate/persistent"]["median"], every["modes"]["plain/loop"]["median"]
    lines.append(f"  sanity: the robust persistent align ({rp:.1f} us) is {'faster' if rp < pl else 'NOT faster'} than the plain "
                 f"launch-per-round loop ({pl:.1f} us)")
    if a.trace:
        for mode in ("cauchy+gate", "huber"):
            lines.append("")
            lines += kernel_trace(tree, mode, a.steps, a.warmup, a.limit)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if all(verdicts) else 2


if __name__ == "__main__":
    sys.exit(main())
