#!/usr/bin/env python3
"""What a round with the pose prior (include/vgicp_hip_prior.h) costs, and that the plain path does not pay for it.  A
developer tool, not a test; the style of tools/probe_robust.py.

The workload is bench.py's C2, resident: synth.make_map(1_000_000), synth.make_uniform_scan(100_000), 20 forced rounds
(translation_sq_threshold 1e-6, cosine_threshold 2.0), >= 200 timed vgicp_align_resident calls per figure after warm-up.

1. The plain path, no prior, on the PARENT's library (--parent, never the tree under test alone) and on the tree's, in
   alternated child processes (parent, tree, parent, tree ...), three of each by default: the median event-measured
   device_seconds per align of every child, on the persistent launch and on the launch-per-round loop.  Accepted when
   the two medians differ by no more than the spread (max - min) of the parent's own repetitions.
2. The prior on the tree's library in one child — plain, a dense prior, and the dense prior with Cauchy 0.15 on top,
   each on the persistent launch and on the loop: device time per round, against the parent's plain round of part 1.

    python tools/probe_prior.py --parent eskf_lio_amd/lib_ab/parent/libvgicp_hip.so --out profiles/r28_prior_timing.txt

Every child runs under its own `timeout -k 10`; the first one that fails ends the run.  A child picks its library
through VGICP_LIB_PATH (eskf_lio_amd/capi.py).
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
ROUNDS = 20
MODES = ("plain", "prior", "prior+cauchy")


def prior_of(guess):
    """A dense information matrix and a prior pose 3 cm / 0.5 degrees off the guess."""
    from eskf_lio_amd import synth
    B = np.random.default_rng(3).normal(size=(6, 6))
    xi = np.array([0.02, -0.02, 0.01, 0.005, -0.005, 0.004])
    return synth.se3_to_SE3(xi) @ guess, 40.0 * (B @ B.T) + 5.0 * np.eye(6)


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
            if mode != "plain":                                  # the parent's library has no such entry point: never called there
                ctx.set_pose_prior(*prior_of(guess))
                if mode == "prior+cauchy":
                    ctx.set_robust("cauchy", 0.15, 0.0)
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
                ctx.clear_pose_prior()
                ctx.set_robust("none", 1.0, 0.0)
        result["fallbacks"] = ctx.counter(1)
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--limit", type=int, default=150, help="seconds a child may take")
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
    every = run_child(tree, MODES, a.steps, a.warmup, a.limit)
    load1 = os.getloadavg()
    lines = [f"tools/probe_prior.py: C2 resident (100 000-point uniform scan, 1 000 000 voxels, {ROUNDS} forced rounds), {a.steps} "
             f"timed aligns after {a.warmup} per figure, event-measured device time, us",
             f"one box: {every['device']}, host {platform.machine()}, load average {load0[0]:.1f} before / {load1[0]:.1f} after",
             f"parent library sha256 {sha256(parent)}", f"tree   library sha256 {sha256(tree)}", "",
             f"1. the plain path, no prior: median device time per align of {a.repeats} alternated child processes each"]
    verdicts, parent_round = [], {}
    for path in ("persistent", "loop"):
        p = [r["modes"][f"plain/{path}"]["median"] for r in series["parent"]]
        t = [r["modes"][f"plain/{path}"]["median"] for r in series["tree"]]
        spread, delta = max(p) - min(p), float(np.median(t) - np.median(p))
        ok = abs(delta) <= spread
        verdicts.append(ok)
        parent_round[path] = float(np.median(p)) / ROUNDS
        lines += [f"  {path:10s} parent " + " ".join(f"{v:8.2f}" for v in p) + f"   median {np.median(p):8.2f}  spread {spread:.2f}",
                  f"  {path:10s} tree   " + " ".join(f"{v:8.2f}" for v in t) + f"   median {np.median(t):8.2f}  "
                  f"difference {delta:+.2f} ({100 * delta / np.median(p):+.2f} %): "
                  f"{'within' if ok else 'BEYOND'} the parent's own spread"]
    lines += ["", "2. the prior on the tree's library, one child: device time per align / per round, against the PARENT's plain round"]
    for key, m in every["modes"].items():
        per_round = m["median"] / m["rounds"]
        base = parent_round[key.split("/")[1]]
        lines.append(f"  {key:24s} {m['median']:8.2f} us per align (p10 {m['p10']:.2f}, p90 {m['p90']:.2f})  {per_round:6.2f} us per round "
                     f"({per_round - base:+.2f} us against the parent's plain {base:.2f})  launches {m['launches']:2d}  "
                     f"counts {m['count_first']} -> {m['count_last']}")
    lines.append(f"  persistent launches that gave up: {every['fallbacks']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if all(verdicts) else 2


if __name__ == "__main__":
    sys.exit(main())
