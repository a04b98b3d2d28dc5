#!/usr/bin/env python3
"""A/B of the scan preparation's host side against another build of the library (a developer tool, not a test).

Two things, both with the parent commit's library given with --parent and the tree's own, each loaded through
VGICP_LIB_PATH in a fresh child process under its own `timeout -k 10`, parent and tree interleaved; the first child that
fails ends the run:

  bits    the prepared scan (kept count, moved count, points, covariances) of every case of tests/prepare_routes_worker.py
          (VGICP_STAGE_LIMIT unset and 1) and of one 60 000-point sweep with 40 states on the staged, the ahead and the
          in-place route, dumped by either library and compared with ==;
  time    host wall time, call to return, of scan_prepare_async and of scan_prepare (ahead route: sweep_stage outside
          the clock, then scan_prepare_staged_async, and that + scan_info) at 60 000 points and 40 states, --steps timed
          calls after --warmup; p50 / p99 per child; who goes first alternates from pair to pair.  Parent against parent shows the run-to-run spread.

    python tools/ab_prepare.py --parent eskf_lio_amd/lib_ab/libvgicp_parent.so --out profiles/r23_prepare_host.txt
"""
import argparse
import hashlib
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, STATES = 60_000, 40


def inputs():
    from eskf_lio_amd import synth
    st = synth.make_imu_states(STATES, seed=STATES)
    t = synth.make_point_times(N, st[1, 0] + 1e-6, st[-3, 0] + 1e-6, seed=9)
    return synth.make_lidar_scan(N, seed=41, extent=30.0), t, st


def worker_time(steps, warmup):
    from eskf_lio_amd import capi
    raw, t, st = inputs()
    out = {"lib": capi.LIB_PATH}
    with capi.Context(0) as ctx:
        def staged_async():
            t0 = time.perf_counter()
            ctx.scan_prepare_async(raw, t, st, None, 0.3, 30)
            dt = time.perf_counter() - t0
            ctx.scan_info()
            return dt

        def staged_sync():
            t0 = time.perf_counter()
            ctx.scan_prepare(raw, t, st, None, 0.3, 30)
            return time.perf_counter() - t0

        def ahead_async():
            ticket = ctx.sweep_stage(raw, t)
            t0 = time.perf_counter()
            ctx.scan_prepare_staged_async(ticket, st, None, 0.3, 30)
            dt = time.perf_counter() - t0
            ctx.scan_info()
            return dt

        def ahead_sync():
            ticket = ctx.sweep_stage(raw, t)
            t0 = time.perf_counter()
            ctx.scan_prepare_staged_async(ticket, st, None, 0.3, 30)
            ctx.scan_info()
            return time.perf_counter() - t0

        for name, call in (("staged_async", staged_async), ("staged_sync", staged_sync), ("ahead_async", ahead_async),
                           ("ahead_sync", ahead_sync)):
            for _ in range(warmup):
                call()
            us = np.array([call() for _ in range(steps)]) * 1e6
            out[name] = {"p50_us": float(np.percentile(us, 50)), "p99_us": float(np.percentile(us, 99)), "calls": steps}
        out["upload_slow"] = ctx.counter(capi.COUNTER_UPLOAD_SLOW)
    print(json.dumps(out), flush=True)


def worker_dump(path):
    """The 60 000-point sweep with 40 states: scan_prepare_async (staged, or in place under VGICP_STAGE_LIMIT=1) and the
    ahead route."""
    from eskf_lio_amd import capi
    raw, t, st = inputs()
    arrays = {}
    with capi.Context(0) as ctx:
        for route in ("direct", "ahead"):
            if route == "direct":
                ctx.scan_prepare_async(raw, t, st, None, 0.3, 30)
            else:
                ctx.scan_prepare_staged_async(ctx.sweep_stage(raw, t), st, None, 0.3, 30)
            kept, moved, _ = ctx.scan_info()
            pts, covs = ctx.scan_download()
            arrays[route + "_counts"], arrays[route + "_pts"], arrays[route + "_cov"] = np.array([kept, moved]), pts.copy(), covs.copy()
    np.savez(path, **arrays)
    print(json.dumps({"lib": capi.LIB_PATH, "dumped": sorted(arrays)}), flush=True)


def child(lib, args, stage_limit=None, seconds=300):
    env = {k: v for k, v in os.environ.items() if k != "VGICP_STAGE_LIMIT"}
    env["VGICP_LIB_PATH"] = os.path.abspath(lib)
    if stage_limit is not None:
        env["VGICP_STAGE_LIMIT"] = stage_limit
    out = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable] + args, capture_output=True, text=True, cwd=ROOT, env=env)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({out.returncode}): {' '.join(args)} with {lib}\n{out.stdout[-2000:]}\n{out.stderr[-3000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=("time", "dump"))
    ap.add_argument("--dump-to")
    ap.add_argument("--parent")
    ap.add_argument("--tree", default=os.path.join(ROOT, "eskf_lio_amd", "lib", "libvgicp_hip.so"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "ab_prepare"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker == "time":
        return worker_time(a.steps, a.warmup)
    if a.worker == "dump":
        return worker_dump(a.dump_to)
    os.makedirs(a.scratch, exist_ok=True)
    me = os.path.abspath(__file__)
    lines = []

    def say(*text):   # every line as it comes: a run that ends early leaves what it had
        lines.extend(text)
        print("\n".join(text), flush=True)

    say(*[f"tools/ab_prepare.py on {platform.node()}, load average {os.getloadavg()}",
             f"parent {a.parent} sha256 {sha(a.parent)}", f"tree   {a.tree} sha256 {sha(a.tree)}", ""])
    # ---- bits ----
    compared = 0
    for limit in (None, "1"):
        files = {}
        for name, lib in (("parent", a.parent), ("tree", a.tree)):
            routes = os.path.join(a.scratch, f"routes_{name}_{limit}.npz")
            big = os.path.join(a.scratch, f"big_{name}_{limit}.npz")
            child(lib, [os.path.join(ROOT, "tests", "prepare_routes_worker.py"), "--dump", routes], limit)
            child(lib, [me, "--worker", "dump", "--dump-to", big], limit)
            files[name] = (np.load(routes), np.load(big))
        for p, t in zip(files["parent"], files["tree"]):
            assert sorted(p.files) == sorted(t.files) and len(p.files) > 0
            for key in p.files:
                if not (p[key].shape == t[key].shape and (p[key] == t[key]).all()):
                    raise SystemExit(f"BITS DIFFER: VGICP_STAGE_LIMIT={limit} {key}")
                compared += 1
        say(f"bits, VGICP_STAGE_LIMIT={limit}: {sum(len(f.files) for f in files['tree'])} arrays of the tree's == the parent's")
    say(f"bits: {compared} arrays compared, all equal", "")
    # ---- time: parent, tree, parent, tree ... ----
    runs = []
    for pair in range(a.pairs):
        order = (("parent", a.parent), ("tree", a.tree))
        for name, lib in order if pair % 2 == 0 else order[::-1]:   # who goes first alternates
            d = child(lib, [me, "--worker", "time", "--steps", str(a.steps), "--warmup", str(a.warmup)], seconds=500)
            runs.append((name, d))
            say(f"time {name} #{pair}: " + "  ".join(f"{k} p50 {v['p50_us']:.1f} p99 {v['p99_us']:.1f} us" for k, v in d.items()
                                                            if isinstance(v, dict)) + f"  upload_slow {d['upload_slow']}")
    say("")
    for key in ("staged_async", "staged_sync", "ahead_async", "ahead_sync"):
        for q in ("p50_us", "p99_us"):
            par = [d[key][q] for name, d in runs if name == "parent"]
            tree = [d[key][q] for name, d in runs if name == "tree"]
            verdict = "inside or below the parent's range" if max(tree) <= max(par) else "ABOVE the parent's range"
            say(f"{key} {q}: parent {min(par):.1f} .. {max(par):.1f}  tree {min(tree):.1f} .. {max(tree):.1f}  ({verdict})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
