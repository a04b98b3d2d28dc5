#!/usr/bin/env python3
"""A/B of vgicp_align_resident_batch against k vgicp_align_resident calls in a row (a developer tool, not a test).

The workload: synth.make_map(50_000), synth.make_structured_scan(27_000, vmap) resident, k in {1, 2, 4, 8} guesses,
20 forced rounds (cosine_threshold = 2.0), >= 300 timed steps after warm-up.  Reported per k: p50 / p99 of the host
wall time of (a) ONE batch call and (b) k single calls in a row, and the event-measured device time of both.

(b), the baseline, is taken on ANOTHER build of the library — the parent commit's, given with --parent — never on
the tree under test alone; the two libraries are timed in interleaved child processes (parent, tree, parent, tree ...),
as DESIGN.md section 7 did for the fused align, and parent against parent shows the run-to-run spread.  Every child runs
under its own `timeout -k 10`; the first one that fails ends the run.

    python tools/ab_align_batch.py --parent eskf_lio_amd/lib_ab/libvgicp_hip_parent.so --out profiles/r20_align_batch.txt

A child talks to its library through ctypes directly (the parent's library has no batch entry points, so capi's
loader is not used for it).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (1, 2, 4, 8)
ROUNDS = 20


def worker(lib_path, mode, steps, warmup):
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
    if mode == "batch":
        lib.vgicp_align_resident_batch.argtypes = [vp, sz, dp, C.POINTER(capi.Params), dp, C.POINTER(capi.BatchStats)]

    def check(ctx, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: status {rc}: {lib.vgicp_last_error(ctx).decode()}")

    f64 = lambda a: a.ctypes.data_as(dp)
    vmap = synth.make_map(50_000)
    pts, covs, _ = synth.make_structured_scan(27_000, vmap)
    pts, covs = np.ascontiguousarray(pts), np.ascontiguousarray(covs)
    rng = np.random.default_rng(5)
    base = np.asarray(synth.GUESS_XI)
    guesses = np.ascontiguousarray(np.stack(
        [capi.pose_to_abi(synth.se3_to_SE3(base + 0.01 * rng.standard_normal(6))) for _ in range(max(KS))]))
    ctx = vp()
    check(None, lib.vgicp_create(0, C.byref(ctx)), "vgicp_create")
    lib.vgicp_device_info.argtypes = [vp, C.c_char_p, sz, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    name, cus, hbm = C.create_string_buffer(64), C.c_int32(), C.c_uint64()
    check(ctx, lib.vgicp_device_info(ctx, name, 64, C.byref(cus), C.byref(hbm)), "vgicp_device_info")
    keys = np.ascontiguousarray(vmap.keys, dtype=np.int32)
    means, mcovs = np.ascontiguousarray(vmap.means), np.ascontiguousarray(vmap.covs)
    check(ctx, lib.vgicp_map_reset(ctx, vmap.voxel_size, keys.shape[0]), "vgicp_map_reset")
    check(ctx, lib.vgicp_map_upsert(ctx, keys.shape[0], keys.ctypes.data_as(C.POINTER(C.c_int32)), f64(means), f64(mcovs)),
          "vgicp_map_upsert")
    check(ctx, lib.vgicp_scan_upload(ctx, pts.shape[0], f64(pts), f64(covs)), "vgicp_scan_upload")
    p = capi.Params(ROUNDS, 0, 1e-6, 2.0, 0, 0)
    out = np.zeros((max(KS), 16))
    result = {"mode": mode, "lib": lib_path, "device": f"{name.value.decode()}, {cus.value} compute units", "k": {}}
    for k in KS:
        st, bst = capi.Stats(), capi.BatchStats()
        gp = [f64(guesses[h]) for h in range(k)]
        op = [f64(out[h]) for h in range(k)]
        wall, dev = [], []
        per_launch = launches = 0
        for step in range(warmup + steps):
            if mode == "batch":
                t0 = time.perf_counter()
                rc = lib.vgicp_align_resident_batch(ctx, k, f64(guesses), C.byref(p), f64(out), C.byref(bst))
                t1 = time.perf_counter()
                check(ctx, rc, "vgicp_align_resident_batch")
                d, per_launch, launches = bst.device_seconds, bst.hypotheses_per_launch, bst.launches
            else:
                d = 0.0
                t0 = time.perf_counter()
                for h in range(k):
                    rc = lib.vgicp_align_resident(ctx, gp[h], C.byref(p), op[h], C.byref(st))
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


def run_child(lib_path, mode, steps, warmup, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib_path,
           "--mode", mode, "--steps", str(steps), "--warmup", str(warmup)]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
        raise SystemExit(f"child ({mode} on {lib_path}) ended with status {proc.returncode}: nothing more is started")
    for line in proc.stdout.splitlines():
        if line.startswith("AB_RESULT "):
            return json.loads(line[len("AB_RESULT "):])
    raise SystemExit("child printed no result")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libvgicp_hip.so of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.join(ROOT, "eskf_lio_amd", "lib", "libvgicp_hip.so"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--mode", choices=("batch", "single"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.lib, a.mode, a.steps, a.warmup)
    if not a.parent:
        raise SystemExit("--parent is required: the baseline is never taken from the tree under test alone")
    if a.steps < 300:
        raise SystemExit("--steps must be at least 300")
    parent, tree = os.path.abspath(a.parent), os.path.abspath(a.tree)
    load0 = os.getloadavg()
    runs = {"parent_a": [], "parent_b": [], "batch": [], "tree_single": []}
    for _ in range(a.pairs):                                   # interleaved: parent, tree, parent, tree's own singles
        runs["parent_a"].append(run_child(parent, "single", a.steps, a.warmup, a.limit))
        runs["batch"].append(run_child(tree, "batch", a.steps, a.warmup, a.limit))
        runs["parent_b"].append(run_child(parent, "single", a.steps, a.warmup, a.limit))
        runs["tree_single"].append(run_child(tree, "single", a.steps, a.warmup, a.limit))
    load1 = os.getloadavg()

    def med(name, k, key):
        return float(np.median([r["k"][str(k)][key] for r in runs[name]]))

    lines = [f"tools/ab_align_batch.py: 27 000-point structured scan against the 50 000-voxel map, {ROUNDS} forced rounds, "
             f"{a.steps} timed steps after {a.warmup}, {a.pairs} interleaved child processes per column (medians over them), us",
             f"one box: {runs['batch'][0]['device']}, host {platform.machine()} with {os.cpu_count()} CPUs, load average "
             f"{load0[0]:.1f} before / {load1[0]:.1f} after",
             f"parent library sha256 {sha256(parent)}", f"tree   library sha256 {sha256(tree)}", "",
             "  k | batch call: p50     p99  device  /launch launches | k single calls, PARENT: p50     p99  device | "
             "parent again p50 | spread | tree's own singles p50 | batch - parent p50"]
    verdict = []
    for k in KS:
        b50, b99, bdev = med("batch", k, "p50"), med("batch", k, "p99"), med("batch", k, "dev_p50")
        pa, pa99, pdev = med("parent_a", k, "p50"), med("parent_a", k, "p99"), med("parent_a", k, "dev_p50")
        pb = med("parent_b", k, "p50")
        ts = med("tree_single", k, "p50")
        per, ln = runs["batch"][0]["k"][str(k)]["per_launch"], runs["batch"][0]["k"][str(k)]["launches"]
        base = 0.5 * (pa + pb)
        spread = abs(pa - pb)
        lines.append(f"{k:3d} | {b50:15.1f} {b99:7.1f} {bdev:7.1f} {per:8d} {ln:8d} | {pa:27.1f} {pa99:7.1f} {pdev:7.1f} | "
                     f"{pb:16.1f} | {spread:6.1f} | {ts:22.1f} | {b50 - base:+.1f}")
        verdict.append((k, per, b50, base, spread))
    lines.append("")
    width = max(per for _, per, _, _, _ in verdict)            # what one launch takes for this scan
    for k, per, b50, base, spread in verdict:
        if k == width and k > 1:
            ok = base - b50 > spread
            lines.append(f"k = {k} = width: the batch's p50 {b50:.1f} us is {'BELOW' if ok else 'NOT below'} the parent's {k} "
                         f"sequential calls ({base:.1f} us) by more than the parent-against-parent spread ({spread:.1f} us): "
                         f"{base - b50:.1f} us less, {base / b50:.2f}x")
    r1 = med("batch", 1, "dev_p50") / ROUNDS
    lines.append(f"device time per round: single launch (batch k = 1 runs vgicp_align_resident) {r1:.2f} us; "
                 + "; ".join(f"k = {k} ({runs['batch'][0]['k'][str(k)]['launches']} launch(es), memset included) "
                             f"{med('batch', k, 'dev_p50') / ROUNDS / runs['batch'][0]['k'][str(k)]['launches']:.2f} us"
                             for k in KS[1:]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
