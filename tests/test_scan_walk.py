"""The resident scan as ONE object that lives through every source, consumer and reader in arbitrary order: seeded walks
over the whole alphabet of tests/scan_walk_reference.py (the walk, the scene, the host model), every synchronous result,
every refusal's status and whole text and every reader of the C ABI held against the model — bit for bit, except the
align's pose against the oracle's (TIGHT_POSE_TOL).

What the walks are for is the host's bookkeeping that the entries share (eskf_lio_amd/csrc/vgicp_context.h): scan_ready,
scan_pending, n and n_upper, the generation, the scan's capacity and the memos behind it, what a preparation found, the
fetch and its checksums, the three staging slots, the keys of a scan made from a map, and which copy carries a deferred
consumer's totals.  tests/test_scan_fetch.py, test_prepare_routes.py, test_fused_tail.py and test_resident_calls.py pin
chosen pairs of entries; a walk runs the sequences nobody thought of.  tests/test_scan_walk_cpu.py holds the conditions
every committed seed meets.

Observed on an MI355X:
  checks per walk   seed 56: 670 plain / 689 raw; seed 1: 674 / 694; seed 22: 676 / 696; seed 11: 670 / 689; seed 1 under
                    VGICP_PERSIST_GRID=2: 674; seed 22 in place (VGICP_STAGE_LIMIT=1, uploads in place): 676.  Each is the
                    number the walk implies (the driver counts them without a device).  A walk takes 0.3 - 0.6 s,
                    the child process 0.9 s.
  conditions        every committed seed carries every condition of tests/test_scan_walk_cpu.py (the fragments of the walk
                    are those sequences; the seeds differ in their order, their readers, the scans' sizes and the map's cap).
  fallbacks         none, in any context of any walk.
  defect found      vgicp_scan_info after a vgicp_preprocess: seed 1, operations 37 .. 39 (prepare_async with deskew,
                    preprocess, scan_info) answered (2977, 0, 0) for (2977, 3963, 0); seed 11, 77 .. 79, (904, 0, 0) for
                    (904, 1013, 0).  resolve_prepare wrote the preprocessed cloud's deskew and indefinite counts into the
                    fields vgicp_scan_info reads.  Fixed (scan_deskewed / scan_indefinite, taken when the resident scan's
                    own preparation is settled); test_a_preprocess_leaves_scan_info_alone keeps the sequence.
  breaks seen       the module built without forget_fetch in begin_scan: seed 56 fails at operation 29 (the fetch_end after
                    an upload of as many points delivers the fetched scan); built with settle_insert reading h_ins_counters
                    always: seed 56 raw fails at operation 6 (the prefix's insertion, whose totals travelled with the first
                    preparation: the raw store's fill stays 0).
"""
import json
import os
import subprocess
import sys

import pytest

import scan_walk_reference as sw
from conftest import TIGHT_POSE_TOL, pose_error
from test_align_batch import assert_same_bits
from test_gpu_parity import _assert_fetch_sums

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def contexts(monkeypatch, raw, upload_in_place=False, **env):
    """The walked context, its twin and the source of vgicp_scan_from_map, all created under `env` (read when a context
    is created, test_launch_variants.py)."""
    from eskf_lio_amd import capi
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    ctx, twin, src = capi.Context(0), capi.Context(0), capi.Context(0)
    for name in env:
        monkeypatch.delenv(name)
    if raw:
        ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)
    if upload_in_place:
        ctx.set_option(capi.OPTION_UPLOAD_STAGE_KB, 0)
    return sw.Device(capi, ctx, twin, src, pose_error, assert_same_bits, TIGHT_POSE_TOL, _assert_fetch_sums)


def run(oracle, monkeypatch, seed, raw, upload_in_place=False, **env):
    device = contexts(monkeypatch, raw, upload_in_place, **env)
    with device.ctx, device.twin, device.src:
        model = sw.run_walk(oracle, seed, raw, device)
        fallbacks = tuple(c.counter(sw.COUNTER_FALLBACKS) for c in (device.ctx, device.twin, device.src))
    return model, fallbacks


def held(model, fallbacks):
    """No launch fell back, and the comparisons that ran are the ones the walk implies."""
    assert fallbacks == (0, 0, 0), fallbacks
    assert model.checks == model.implied > sw.WALK_LENGTH * 3, (model.checks, model.implied)
    print(f"{model.checks} checks")


@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
@pytest.mark.parametrize("seed", sw.SEEDS)
def test_walk(oracle, monkeypatch, seed, raw):
    """120 operations, a full check of every reader at every 8th and single readers in between; with the raw-point store,
    the per-voxel lists too (the deferred consumers' totals travel with two more words then)."""
    held(*run(oracle, monkeypatch, seed, raw))


def test_walk_with_several_points_per_thread(oracle, monkeypatch):
    """VGICP_PERSIST_GRID=2: the persistent launch has two workgroups, so every scan of the walk gives a thread several
    points and the align's memos live in d_memo — which is reallocated with the scan's memory."""
    held(*run(oracle, monkeypatch, sw.SEEDS[1], False, VGICP_PERSIST_GRID="2"))


def test_walk_in_place(oracle):
    """VGICP_STAGE_LIMIT=1 (read once per process: a child), so that every preparation that is not staged ahead takes the
    in-place route, and VGICP_OPTION_UPLOAD_STAGE_KB = 0 for the uploads."""
    env = dict(os.environ, VGICP_STAGE_LIMIT="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scan_walk_reference.py"), str(sw.SEEDS[2]), "plain"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    print(d)
    assert d["stage_limit"] == "1" and d["fallbacks"] == [0, 0, 0] and d["checks"] == d["implied"] > sw.WALK_LENGTH * 3


# ---- what the walks found, kept as the sequence that showed it ---------------------------------------------------------
def test_a_preprocess_leaves_scan_info_alone(oracle, gpu_ctx):
    """vgicp_preprocess does not touch the resident scan, so vgicp_scan_info must go on describing that scan.  It used to
    answer with the deskew count and the indefinite count of the cloud that was preprocessed in between (resolve_prepare
    wrote both into the fields vgicp_scan_info reads): (kept, 0, ..) for a deskewed resident scan.  The counter
    VGICP_COUNTER_PREP_INDEFINITE is the last preparation's, vgicp_preprocess included, as its comment says."""
    scene = sw.Scene(oracle, 1)
    sweep = scene.sweep(0, ext=True, deskew=True)
    other = scene.sweep(1)
    assert sweep.info[1] > 0
    gpu_ctx.scan_prepare_async(sweep.raw, sweep.times, sweep.states, sweep.extrinsic, sw.PREP_VOXEL, sw.KNN)
    kept, _, _ = gpu_ctx.preprocess(other.raw, 0.4, sw.KNN)
    assert len(kept) == len(oracle.preprocess(other.raw, 0.4, sw.KNN)[0])
    assert gpu_ctx.scan_info() == sweep.info
    gp, gc = gpu_ctx.scan_download()
    assert sw.same_bits(gp, sweep.scan.points) and sw.same_bits(gc, sweep.scan.covs)
    assert gpu_ctx.counter(4) == oracle.preprocess_ex(other.raw, 0.4, sw.KNN)[3]
    gpu_ctx.deskew(other.raw, other.times, scene.states)
    assert gpu_ctx.scan_info() == sweep.info
