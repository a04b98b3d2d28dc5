#!/usr/bin/env python3
"""A/B of vgicp_evaluate_resident against the cheapest way the parent commit's library offers to get part of its answer:
k calls of vgicp_align_resident with max_iteration = 1 (count and normal equations of the pose, no cost, no squared
error).  A developer tool, not a test.

The workload: synth.make_map(50_000), synth.make_structured_scan(27_000, vmap) resident, k in {1, 4, 16, 64} poses,
>= 300 timed steps after warm-up.  Reported per k: p50 / p99 of the host wall time of (a) ONE vgicp_evaluate_resident
call on the tree's library and (b) k one-round aligns in a row on the PARENT's library (given with --parent, never the
tree under test alone), and the event-measured device time of both.  The two libraries are timed in interleaved child
processes (parent, tree, parent ...); parent against parent shows the run-to-run spread.  Every child runs under its
own `timeout -k 10`; the first one that fails ends the run.

    python tools/ab_evaluate.py --parent eskf_lio_amd/lib_ab/libvgicp_hip_parent.so --out profiles/r21_evaluate.txt

--trace runs ONE child of the tree's library (k = 16) under `rocprofv3 --kernel-trace --stats`, a run of its own, and
appends the two kernels' rows of the statistics to the report.

A child talks to its library through ctypes directly (the parent's library has no vgicp_evaluate_resident, so capi's
loader is not used for it).
"""
import argparse
import ctypes as C
import csv
import glob
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
KS = (1, 4, 16, 64)


def worker(lib_path, mode, steps, warmup, ks):
    from eskf_lio_amd import capi, synth
    lib = C.CDLL(lib_path, mode=C.RTLD_GLOBAL)
    vp, dp, sz = C.c_void_p, C.POINTER(C.c_double), C.c_size_t
    lib.vgicp_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.vgicp_destroy.argtypes = [vp]
    lib.vgicp_last_error.argtypes = [vp]
    lib.vgicp_last_error.restype = C.c_char_p
    lib.vgicp_map_reset.argtypes = [vp, C.c_double, sz]
    lib.vgicp_map_upsert.argtypes = [vp, sz, C.POINTER(C.c_int32), dp, dp]
    lib.vgicp_scan_upload.argtypes = [vp, sz, dp, dp]
    lib.vgicp_align_resident.argtypes = [vp, dp, C.POINTER(capi.Params), dp, C.POINTER(capi.Stats)]
    lib.vgicp_device_info.argtypes = [vp, C.c_char_p, sz, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    if mode == "evaluate":
        lib.vgicp_evaluate_resident.argtypes = [vp, sz, dp, C.POINTER(capi.Evaluation), C.POINTER(capi.EvalStats)]

    def check(ctx, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: status {rc}: {lib.vgicp_last_error(ctx).decode()}")

    f64 = lambda a: a.ctypes.data_as(dp)
    vmap = synth.make_map(50_000)
    pts, covs, _ = synth.make_structured_scan(27_000, vmap)
    pts, covs = np.ascontiguousarray(pts), np.ascontiguousarray(covs)
    rng = np.random.default_rng(5)
    base = np.asarray(synth.GUESS_XI)
    poses = np.ascontiguousarray(np.stack(
        [capi.pose_to_abi(synth.se3_to_SE3(base + 0.01 * rng.standard_normal(6))) for _ in range(max(KS))]))
    ctx = vp()
    check(None, lib.vgicp_create(0, C.byref(ctx)), "vgicp_create")
    name, cus, hbm = C.create_string_buffer(64), C.c_int32(), C.c_uint64()
    check(ctx, lib.vgicp_device_info(ctx, name, 64, C.byref(cus), C.byref(hbm)), "vgicp_device_info")
    keys = np.ascontiguousarray(vmap.keys, dtype=np.int32)
    means, mcovs = np.ascontiguousarray(vmap.means), np.ascontiguousarray(vmap.covs)
    check(ctx, lib.vgicp_map_reset(ctx, vmap.voxel_size, keys.shape[0]), "vgicp_map_reset")
    check(ctx, lib.vgicp_map_upsert(ctx, keys.shape[0], keys.ctypes.data_as(C.POINTER(C.c_int32)), f64(means), f64(mcovs)),
          "vgicp_map_upsert")
    check(ctx, lib.vgicp_scan_upload(ctx, pts.shape[0], f64(pts), f64(covs)), "vgicp_scan_upload")
    p = capi.Params(1, 0, 1e-6, 2.0, 0, 0)                     # one round: count and normal equations of the pose
    out = np.zeros(16)
    evs = (capi.Evaluation * max(KS))()
    result = {"mode": mode, "lib": lib_path, "device": f"{name.value.decode()}, {cus.value} compute units", "k": {}}
    for k in ks:
        st, est = capi.Stats(), capi.EvalStats()
        gp = [f64(poses[h]) for h in range(k)]
        wall, dev = [], []
        per_launch = launches = 0
        for step in range(warmup + steps):
            if mode == "evaluate":
                t0 = time.perf_counter()
                rc = lib.vgicp_evaluate_resident(ctx, k, f64(poses), evs, C.byref(est))
                t1 = time.perf_counter()
                check(ctx, rc, "vgicp_evaluate_resident")
                d, per_launch, launches = est.device_seconds, est.poses_per_launch, est.launches
            else:
                d = 0.0
                t0 = time.perf_counter()
                for h in range(k):
                    rc = lib.vgicp_align_resident(ctx, gp[h], C.byref(p), f64(out), C.byref(st))
                    if rc != 0:
                        break
                    d += st.device_seconds
                t1 = time.perf_counter()
                check(ctx, rc, "vgicp_align_resident")
                per_launch, launches = 1, k * st.launches
            if step >= warmup:
                wall.append((t1 - t0) * 1e6)
                dev.append(d * 1e6)
        w, d = np.asarray(wall), np.asarray(dev)
        result["k"][str(k)] = dict(p50=float(np.percentile(w, 50)), p99=float(np.percentile(w, 99)),
                                   dev_p50=float(np.percentile(d, 50)), dev_p99=float(np.percentile(d, 99)),
                                   per_launch=int(per_launch), launches=int(launches), steps=len(wall))
    lib.vgicp_destroy(ctx)
    print("AB_RESULT " + json.dumps(result), flush=True)


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def child_command(lib_path, mode, steps, warmup, ks):
    return [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib_path, "--mode", mode, "--steps", str(steps),
            "--warmup", str(warmup), "--ks", ",".join(str(k) for k in ks)]


def run_child(lib_path, mode, steps, warmup, limit):
    cmd = ["timeout", "-k", "10", str(limit)] + child_command(lib_path, mode, steps, warmup, KS)
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
        raise SystemExit(f"child ({mode} on {lib_path}) ended with status {proc.returncode}: nothing more is started")
    for line in proc.stdout.splitlines():
        if line.startswith("AB_RESULT "):
            return json.loads(line[len("AB_RESULT "):])
    raise SystemExit("child printed no result")


def kernel_trace(tree, steps, warmup, limit):
    """One child (k = 16) under rocprofv3 --kernel-trace --stats; -> report lines for the two kernels."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
               "-d", tmp, "--"] + child_command(tree, "evaluate", steps, warmup, (16,))
        proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if proc.returncode != 0:
            sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
            raise SystemExit(f"the traced child ended with status {proc.returncode}")
        lines = [f"rocprofv3 --kernel-trace --stats, a run of its own: {warmup + steps} calls of k = 16 (one launch pair each)"]
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "evaluate" in row.get("Name", ""):
                    short = "evaluate_fold_kernel" if "fold" in row["Name"] else "evaluate_kernel<512>"
                    lines.append(f"  {short:22s} calls {row.get('Calls')}  average {float(row.get('AverageNs', 'nan')) / 1e3:.2f} us  "
                                 f"min {float(row.get('MinNs', 'nan')) / 1e3:.2f}  max {float(row.get('MaxNs', 'nan')) / 1e3:.2f}")
        if len(lines) == 1:
            lines.append("  (no kernel statistics found in the profiler's output)")
        return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libvgicp_hip.so of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.join(ROOT, "eskf_lio_amd", "lib", "libvgicp_hip.so"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--trace", action="store_true", help="also one child under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--mode", choices=("evaluate", "align1"))
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    a = ap.parse_args()
    if a.worker:
        return worker(a.lib, a.mode, a.steps, a.warmup, tuple(int(k) for k in a.ks.split(",")))
    if not a.parent:
        raise SystemExit("--parent is required: the baseline is never taken from the tree under test alone")
    if a.steps < 300:
        raise SystemExit("--steps must be at least 300")
    parent, tree = os.path.abspath(a.parent), os.path.abspath(a.tree)
    load0 = os.getloadavg()
    runs = {"parent_a": [], "parent_b": [], "evaluate": []}
    for _ in range(a.pairs):                                   # interleaved: parent, tree, parent
        runs["parent_a"].append(run_child(parent, "align1", a.steps, a.warmup, a.limit))
        runs["evaluate"].append(run_child(tree, "evaluate", a.steps, a.warmup, a.limit))
        runs["parent_b"].append(run_child(parent, "align1", a.steps, a.warmup, a.limit))
    load1 = os.getloadavg()

    def med(name, k, key):
        return float(np.median([r["k"][str(k)][key] for r in runs[name]]))

    lines = [f"tools/ab_evaluate.py: 27 000-point structured scan against the 50 000-voxel map, {a.steps} timed steps after "
             f"{a.warmup}, {a.pairs} interleaved child processes per column (medians over them), us",
             f"one box: {runs['evaluate'][0]['device']}, host {platform.machine()} with {os.cpu_count()} CPUs, load average "
             f"{load0[0]:.1f} before / {load1[0]:.1f} after",
             f"parent library sha256 {sha256(parent)}", f"tree   library sha256 {sha256(tree)}", "",
             "  k | ONE vgicp_evaluate_resident: p50     p99  device  /launch launches | k one-round aligns, PARENT: p50     p99  "
             "device | parent again p50 | spread | ratio"]
    for k in KS:
        e50, e99, edev = med("evaluate", k, "p50"), med("evaluate", k, "p99"), med("evaluate", k, "dev_p50")
        pa, pa99, pdev = med("parent_a", k, "p50"), med("parent_a", k, "p99"), med("parent_a", k, "dev_p50")
        pb = med("parent_b", k, "p50")
        per, ln = runs["evaluate"][0]["k"][str(k)]["per_launch"], runs["evaluate"][0]["k"][str(k)]["launches"]
        lines.append(f"{k:3d} | {e50:32.1f} {e99:7.1f} {edev:7.1f} {per:8d} {ln:8d} | {pa:31.1f} {pa99:7.1f} {pdev:7.1f} | "
                     f"{pb:16.1f} | {abs(pa - pb):6.1f} | {0.5 * (pa + pb) / e50:.2f}x")
    lines.append("")
    one = 0.5 * (med("parent_a", 1, "p50") + med("parent_b", 1, "p50"))
    lines.append(f"16 poses in one call: {med('evaluate', 16, 'p50'):.1f} us, against {one:.1f} us for ONE one-round align on the "
                 f"parent ({med('evaluate', 16, 'p50') / one:.2f}x)")
    if a.trace:
        lines.append("")
        lines += kernel_trace(tree, a.steps, a.warmup, a.limit)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
