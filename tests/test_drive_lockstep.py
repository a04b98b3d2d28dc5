"""The street drive (BASELINE config C4's stand-in) frame by frame against the oracle, in lockstep.

tests/test_replay.py::test_street_drive_c4_surrogate compares two closed loops, which drift apart once a point lands on
the other side of a voxel face, so its bounds loosen after frame 10.  Here every frame starts both chains from the same
state instead (teacher forcing, tests/replay_backends.py LockstepBackend): the device prepares the sweep, the oracle
aligns and inserts the device's prepared scan, both align from the same guess and must agree round by round, the
oracle's pose goes back to the filter, both maps take the same insertion and eviction and are compared bit for bit
after every eviction, every rehash and at the end.  A frame may part only with a certificate (certify_divergence).

GPU part: four device chains over the drive.  CPU part: the harness itself, against a stand-in "device" built from
the oracle into which single small errors are injected: each must make the lockstep fail."""
import hashlib
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest

from eskf_lio_amd import replay, synth
from replay_backends import LockstepBackend, certify_divergence, first_difference, reference_prepare


def _drive_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_drive_fixture", os.path.join(os.path.dirname(__file__), "golden", "make_drive_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(cfg, backend, events):
    odo = replay.Odometry(cfg, backend)
    traj = odo.run(events)
    backend.finish()
    return traj


# ---- GPU: the four device chains ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)   # measured: 25 s / 27 s / 25 s / 25 s
@pytest.mark.parametrize("variant", ["resident", "dense", "enqueued_reference_order", "two_sub_contexts"])
def test_street_drive_lockstep(capsys, monkeypatch, oracle, variant):
    """`resident`: replay.DeviceBackend(cfg, 0) as the product runs it (vgicp_scan_prepare -> vgicp_align_resident ->
    vgicp_map_insert_resident -> vgicp_map_evict).  `dense`: the persistent launch on 120 workgroups with the
    dense-copy threshold at 4 096 slots (several points per thread; the dense record copy rebuilt every frame).
    `enqueued_reference_order`: VGICP_OPTION_REFERENCE_ORDER on, through vgicp_scan_prepare_async -> vgicp_scan_fetch
    -> vgicp_align_resident -> vgicp_map_insert_resident_async.  `two_sub_contexts`: one
    multi-device context of two sub-contexts on device 0 (replicated map, point-sharded align).
    Every run: 300 frames, the table grows through >= 3 sizes, an eviction fires, every frame meets the tight bounds
    or is certified (<= 2).  Outside the reference order the lockstep chain IS the oracle chain that made
    tests/golden/drive_c4.npz (its inputs are the device's prepared scans, which must equal the oracle's), so it must
    reproduce that file: round counts, kept and removed counts and stamps exactly, poses to 1e-9, the final voxel set
    and count sum exactly."""
    if variant == "dense":
        monkeypatch.setenv("VGICP_PERSIST_GRID", "120")
        monkeypatch.setenv("VGICP_DENSE_SLOTS", "4096")
    frames = 300
    mod = _drive_module()
    cfg = mod.drive_config()
    device = replay.DeviceBackend(cfg, [0, 0] if variant == "two_sub_contexts" else 0)
    lines = []
    lock = LockstepBackend(cfg, oracle, device, enqueued=variant.startswith("enqueued"),
                           reference_order=variant.endswith("reference_order"), log=lines.append)
    t0 = time.perf_counter()
    try:
        traj = _run(cfg, lock, mod.lazy_events(frames))
        with capsys.disabled():
            print(f"\n[lockstep {variant}: {len(traj)} frames in {time.perf_counter() - t0:.0f} s; map comparisons "
                  f"{[w for _, w in lock.map_checks]}; preparations compared at frames {sorted(set(lock.prep_checks))}; "
                  f"table sizes {sorted(lock.slots_seen)}; largest pose difference {max(lock.pose_diff):.3e}; "
                  f"accepted {len(lock.accepted)}]")
        assert len(traj) == frames
        assert len(lock.slots_seen) >= 3, lock.slots_seen
        assert len(lock.removed) >= 1 and sum(w == "eviction" for _, w in lock.map_checks) == len(lock.removed)
        assert len(lock.accepted) <= 2
        if variant != "two_sub_contexts":
            assert device.ctx.counter(1) == 0                  # no persistent launch gave up
        if variant == "dense":
            assert device.ctx.counter(0) >= frames - 1          # every align was one persistent launch
        if variant != "enqueued_reference_order":
            ref = np.load(os.path.join(os.path.dirname(__file__), "golden", "drive_c4.npz"))
            assert int(ref["frames"]) == frames
            assert [s for s, _ in traj] == ref["stamps"].tolist()
            dev = max(max(abs(a - b) for a, b in zip(T.ravel(), R.ravel())) for (_, T), R in zip(traj, ref["poses"]))
            assert dev <= 1e-9, dev
            assert lock.iterations == ref["iterations"].tolist()
            assert lock.kept == ref["kept"].tolist()
            assert lock.removed == ref["removed"].tolist()
            keys, _, _, counts = device.ctx.map_export()
            assert np.array_equal(keys, ref["map_keys"]) and int(counts.sum()) == int(ref["map_count_sum"])
    finally:
        with capsys.disabled():
            for line in lines:                                  # every accepted divergence, also when the run failed
                print(line)
        device.ctx.close()


# ---- CPU: the harness against a stand-in device made of the oracle -----------------------------------------------
class _PrepCache:
    """The oracle's preparation of a sweep, once per distinct input (the teacher-forced chain feeds every run the
    same sweeps and states, so a whole module of runs prepares each frame once)."""

    def __init__(self, oracle, cfg):
        self.o, self.cfg, self.memo = oracle, cfg, {}

    def __call__(self, states, points, pointTime):
        h = hashlib.sha1()
        for a in (states, points, pointTime):
            h.update(b"-" if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes())
        key = h.hexdigest()
        if key not in self.memo:
            self.memo[key] = reference_prepare(self.o, np.asarray(self.cfg["lidar_extrinsic"]),
                                               self.cfg["cloud_preprocessor"]["voxel_size"], states, points, pointTime)
        return self.memo[key]


class OracleContext:
    """capi.Context's frame-chain calls on the oracle, with one fault to inject:
    ulp_mean (a voxel's mean one ulp off after the n-th insertion), drop (frame, round): one point fewer in that round,
    evict_short (the eviction count one too small), swap (frame): the downloaded scan with two points swapped."""

    def __init__(self, oracle, prepare, fault=None, at=None):
        self.o, self.prepare, self.fault, self.at = oracle, prepare, fault, at
        self.map, self.slots, self.frame, self.inserts, self.nudged = None, 0, -1, 0, None

    def map_reset(self, voxel_size, capacity_hint=0):
        self.voxel, self.map = voxel_size, None

    def scan_prepare(self, points, point_time, states, extrinsic, voxel, knn):
        self.frame += 1
        self.scan = self.prepare(states, points, point_time)
        return len(self.scan[0]), 0

    def scan_download(self):
        p, c = self.scan[0].copy(), self.scan[1].copy()
        if self.fault == "swap" and self.frame == self.at:
            p[[10, 11]], c[[10, 11]] = p[[11, 10]], c[[11, 10]]
        return p, c

    def align_resident(self, guess, max_iteration, translation_sq_threshold, cosine_threshold):
        if self.fault == "drop" and self.frame == self.at[0]:
            return self._gauss_newton(guess, max_iteration, translation_sq_threshold, cosine_threshold, self.at[1])
        return self.map.align(*self.scan, guess, max_iteration, translation_sq_threshold, cosine_threshold)

    def _gauss_newton(self, guess, max_iteration, t_thr, c_thr, drop_round):
        """oracle_align's loop in Python, with one matched point left out of round drop_round."""
        p, c = self.o.transform(*self.scan, guess)
        total, counts, jtj, jtr, converged = np.asarray(guess, dtype=np.float64).copy(), [], [], [], False
        for it in range(max_iteration):
            keep = np.ones(len(p), dtype=bool)
            if it == drop_round:
                full = self.map.accumulate(p, c)[2]
                for k in range(len(p)):
                    keep[k] = False
                    if self.map.accumulate(p[keep], c[keep])[2] == full - 1:
                        break
                    keep[k] = True
            J, r, m = self.map.accumulate(p[keep], c[keep])
            counts.append(m), jtj.append(J), jtr.append(r)
            _, step = self.o.solve_step(J, r)
            total = step @ total
            if self.o.convergence_check(step, c_thr, t_thr):
                converged = True
                break
            p, c = self.o.transform(p, c, step)
        return SimpleNamespace(pose=total, iterations=len(counts), converged=converged, corr_count=np.array(counts),
                               JTJ=np.array(jtj), JTr=np.array(jtr))

    def map_insert_resident(self, transform, max_points_per_voxel):
        if self.map is None:
            self.map = self.o.OracleMap(self.voxel, max_points_per_voxel)
        self.map.insert(*self.o.transform(*self.scan, transform))
        self.inserts += 1
        if self.fault == "ulp_mean" and self.inserts == self.at:
            keys = self.map.export()[0]
            self.nudged = tuple(keys[len(keys) // 2].tolist())

    def map_evict(self, position, distance_threshold):
        n = self.map.evict(position, distance_threshold)
        return n - 1 if self.fault == "evict_short" else n

    def map_size(self):
        n = len(self.map) if self.map is not None else 0
        while self.slots < 2 * n:                                # a table that doubles at half load
            self.slots = max(2 * self.slots, 1024)
        return n, self.slots

    def map_export(self):
        keys, means, covs, counts = self.map.export()
        order = np.lexsort(keys.T)
        keys, means, covs, counts = keys[order], means[order].copy(), covs[order], counts[order]
        if self.nudged is not None:
            i = [tuple(k) for k in keys.tolist()].index(self.nudged)
            means[i, 0] = np.nextafter(means[i, 0], np.inf)
        return keys, means, covs, counts

    def counter(self, which):
        return 0


@pytest.fixture(scope="module")
def short_drive(oracle):
    """8 sweeps of the drive, evicted every 2 map updates at 25 m so that evictions remove voxels."""
    cfg = _drive_module().drive_config()
    cfg["local_map"].update(distance_threshold=25.0, remove_every_updates=2)
    raw = list(synth.iter_drive_stream(frames=8))
    return cfg, raw, _PrepCache(oracle, cfg)


def _lockstep(oracle, short_drive, fault=None, at=None):
    from replay_backends import stream_events
    cfg, raw, prep = short_drive
    lock = LockstepBackend(cfg, oracle, SimpleNamespace(ctx=OracleContext(oracle, prep, fault, at)), prepare=prep,
                           log=lambda s: None)
    traj = _run(cfg, lock, stream_events(replay, raw))
    return lock, traj


@pytest.mark.timeout(300)   # measured: 7 s on 8 cores (the first test prepares the 8 sweeps)
def test_lockstep_passes_on_an_exact_device(oracle, short_drive):
    lock, traj = _lockstep(oracle, short_drive)
    assert len(traj) == 8 and lock.accepted == []
    assert max(lock.pose_diff) == 0.0
    assert len(lock.removed) >= 2 and min(lock.removed) > 0       # evictions fired and removed voxels
    whys = [w for _, w in lock.map_checks]
    assert whys.count("eviction") == len(lock.removed) and whys[-1] == "final" and "rehash" in whys
    assert {0, 1}.issubset(lock.prep_checks)


@pytest.mark.timeout(120)   # measured: 0.1-0.2 s each (the sweeps come prepared)
@pytest.mark.parametrize("fault,at,message", [
    ("ulp_mean", 2, r"means differ in 1 voxels"),
    ("drop", (3, 0), r"frame 3: round 0: \d+ correspondences on the device.*no point changes voxel"),
    ("evict_short", None, r"eviction removed"),
    ("swap", 1, r"frame 1: prepared scans differ in 2 rows"),
])
def test_lockstep_catches_a_small_device_error(oracle, short_drive, fault, at, message):
    with pytest.raises(AssertionError, match=message):
        _lockstep(oracle, short_drive, fault, at)


def _built_case(oracle, shift):
    """One align pair on a 0.25 m grid (faces at exact binary fractions): the device's entry pose for round 1 is the
    oracle's moved by `shift` along x; the point sits 1e-13 m below the face x = 2.0 under the oracle's pose."""
    pts = np.array([[2.0 - 1e-13, 0.1, 0.1], [0.6, 0.6, 0.6]])
    po = np.eye(4)
    pd = np.eye(4)
    pd[0, 3] = shift
    J = np.tile(np.eye(6), (3, 1, 1))
    ora = SimpleNamespace(pose=po, iterations=3, converged=True, corr_count=np.array([10, 10, 10]), JTJ=J, JTr=np.zeros((3, 6)))
    dev = SimpleNamespace(pose=pd, iterations=3, converged=True, corr_count=np.array([10, 11, 11]), JTJ=J, JTr=np.zeros((3, 6)))
    reg = dict(translation_sq_threshold=1e-6, cosine_threshold=0.9999)
    return certify_divergence(oracle, 0.25, pts, np.eye(4), dev, ora, lambda k: SimpleNamespace(pose=pd),
                              lambda k: SimpleNamespace(pose=po), reg)


def test_certificate_accepts_a_point_on_a_voxel_face(oracle):
    cert = _built_case(oracle, 1e-12)
    assert cert["accepted"] and cert["kind"] == "voxel face" and cert["round"] == 1, cert
    assert cert["points"] == [0] and cert["distances"][0] <= 2e-13


def test_certificate_rejects_a_pose_difference_without_a_face(oracle):
    cert = _built_case(oracle, 1e-6)
    assert not cert["accepted"] and "apart" in cert["why"], cert
    # the same 1e-6 m with the point far from any face: no tie explains it either way
    pts = np.array([[2.1, 0.1, 0.1]])
    J = np.tile(np.eye(6), (2, 1, 1))
    ora = SimpleNamespace(iterations=2, converged=True, corr_count=np.array([5, 5]), JTJ=J, JTr=np.zeros((2, 6)))
    dev = SimpleNamespace(iterations=2, converged=True, corr_count=np.array([5, 6]), JTJ=J, JTr=np.zeros((2, 6)))
    pd = np.eye(4)
    pd[0, 3] = 1e-6
    cert = certify_divergence(oracle, 0.25, pts, np.eye(4), dev, ora, lambda k: SimpleNamespace(pose=pd),
                              lambda k: SimpleNamespace(pose=np.eye(4)), dict(translation_sq_threshold=1e-6, cosine_threshold=0.9999))
    assert not cert["accepted"], cert
    assert first_difference(dev, ora)[0] == 1
