"""vgicp_align_resident_batch (include/vgicp_hip_batch.h): one resident scan registered from several guesses, the
hypotheses side by side as teams of ONE persistent launch.

The contract is bit equality with vgicp_align_resident on the same context state, so every comparison with the single
call is `==` / np.array_equal; poses and counts are also held against the CPU oracle with assert_align_parity's bounds.
"""
import numpy as np
import pytest

from conftest import POSE_TOL_M, POSE_TOL_RAD, TIGHT_POSE_TOL, pose_error

pytestmark = pytest.mark.gpu

TSQ, COS = 1e-6, 0.9999            # the shipped thresholds
# the fan of the issue's table: right basin three times (3, 2 and 4 rounds on the oracle), a wrong basin once (no
# convergence within 20 rounds)
FAN_XI = ([0.0] * 6, [0.04, -0.02, 0.008, 0.0, 0.0, 0.008], [-0.064, 0.032, 0.0, 0.008, 0.0, -0.024],
          [0.6, 0.5, 0.3, 0.0, 0.0, 0.2])


def assert_align_parity(got, ref, tight=TIGHT_POSE_TOL):
    """tests/test_gpu_parity.py's bounds."""
    assert got.iterations == ref.iterations
    assert got.converged == ref.converged
    assert np.array_equal(got.corr_count, ref.corr_count)
    dt, dr = pose_error(got.pose, ref.pose)
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert dt <= tight and dr <= tight


def assert_same_bits(got, want, what=""):
    assert got.status == want.status, what
    assert got.iterations == want.iterations and got.converged == want.converged, (what, got.iterations, want.iterations)
    assert np.array_equal(got.pose, want.pose, equal_nan=True), what
    assert np.array_equal(got.corr_count, want.corr_count), what
    assert np.array_equal(got.normal_eq, want.normal_eq, equal_nan=True), what


def singles(ctx, guesses, max_it, tsq, cos, flags=0):
    return [ctx.align_resident(g, max_it, tsq, cos, flags=flags, allow_degenerate=True) for g in guesses]


def assert_batch_equals_singles(ctx, guesses, max_it, tsq, cos, flags=0, what=""):
    want = singles(ctx, guesses, max_it, tsq, cos, flags)
    got = ctx.align_resident_batch(guesses, max_it, tsq, cos, flags=flags)
    assert len(got) == len(want) == len(guesses)
    for h in range(len(guesses)):
        assert_same_bits(got[h], want[h], f"{what} hypothesis {h} of {len(guesses)}")
    return got, want


def load_map(ctx, vmap):
    ctx.map_reset(vmap.voxel_size, vmap.keys.shape[0])
    ctx.map_upsert(vmap.keys, vmap.means, vmap.covs)


def grid_of(ctx):
    return min(ctx.device_info()[1], 256)      # as vgicp_create sets it


def expected_width(ctx, n):
    return min(16, grid_of(ctx) // -(-n // 448))


def jitter_guesses(k, seed=5):
    """k distinct small perturbations of the default guess."""
    from eskf_lio_amd import synth
    rng = np.random.default_rng(seed)
    base = np.asarray(synth.GUESS_XI, dtype=np.float64)
    return [synth.se3_to_SE3(base + 0.01 * rng.standard_normal(6)) for _ in range(k)]


@pytest.fixture(scope="module")
def fan_inputs():
    from eskf_lio_amd import synth
    vmap = synth.make_map(50_000)
    pts, covs, _ = synth.make_structured_scan(27_000, vmap)
    return vmap, pts, covs, [synth.se3_to_SE3(xi) for xi in FAN_XI]


@pytest.fixture()
def fan_ctx(gpu_ctx, fan_inputs):
    vmap, pts, covs, _ = fan_inputs
    load_map(gpu_ctx, vmap)
    gpu_ctx.scan_upload(pts, covs)
    return gpu_ctx


# ---- 1 -------------------------------------------------------------------------------------------------------------
def test_fan_of_four_runs_in_one_launch_with_the_single_calls_bits(fan_ctx, fan_inputs, oracle):
    vmap, pts, covs, guesses = fan_inputs
    got, want = assert_batch_equals_singles(fan_ctx, guesses, 20, TSQ, COS, what="fan")
    if fan_ctx.device_info()[1] == 256:
        assert got.hypotheses_per_launch == 4 and got.launches == 1
        assert fan_ctx.align_batch_width() == 4
    if got.hypotheses_per_launch > 1:                       # side by side: one synchronisation for the whole fan
        fan_ctx.frame_stats(reset=True)
        again = fan_ctx.align_resident_batch(guesses, 20, TSQ, COS)
        fs = fan_ctx.frame_stats()
        assert fs.host_syncs == 1 and fs.kernel_launches == again.launches
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    refs = [om.align(pts, covs, g, 20, TSQ, COS) for g in guesses]
    for h, ref in enumerate(refs):
        assert_align_parity(got[h], ref)
    # teams that leave the launch in different rounds are what this test is about
    assert len({r.iterations for r in refs}) > 1
    assert [r.iterations for r in got] == [r.iterations for r in refs]
    assert not refs[3].converged and not got[3].converged and refs[3].iterations == 20


# ---- 2 -------------------------------------------------------------------------------------------------------------
def test_a_hypothesis_does_not_depend_on_its_neighbours(fan_ctx, fan_inputs):
    _, _, _, guesses = fan_inputs
    probe = guesses[2]
    want = fan_ctx.align_resident(probe, 20, TSQ, COS)
    others = [guesses[0], guesses[1], guesses[3]]
    for pos in range(4):                                    # every position of a batch of four
        batch = others[:pos] + [probe] + others[pos:]
        got = fan_ctx.align_resident_batch(batch, 20, TSQ, COS)
        assert_same_bits(got[pos], want, f"position {pos}")
    fill = jitter_guesses(8) + [guesses[3]]
    for k in (1, 2, 3, 4, 5, 9):                            # 9: more than one launch
        for pos in sorted({0, k // 2, k - 1}):
            batch = [fill[i] for i in range(k)]
            batch[pos] = probe
            got = fan_ctx.align_resident_batch(batch, 20, TSQ, COS)
            assert len(got) == k
            assert_same_bits(got[pos], want, f"k {k} position {pos}")
            if k == 9 and got.hypotheses_per_launch > 1:
                assert got.launches == -(-9 // got.hypotheses_per_launch)


# ---- 3 -------------------------------------------------------------------------------------------------------------
def test_team_geometry_edges(c1_gpu, c1_inputs):
    from eskf_lio_amd import synth
    vmap, _, _ = c1_inputs
    grid = grid_of(c1_gpu)
    widest_two = (grid // 2) * 448                          # the largest scan that still leaves room for two teams
    sizes = [1, 447, 448, 449, 16 * 448 + 1, widest_two, widest_two + 1]
    guesses = jitter_guesses(16)                            # as many as the widest launch takes
    for n in sizes:
        pts, covs = synth.make_uniform_scan(n, vmap)
        c1_gpu.scan_upload(pts, covs)
        width = expected_width(c1_gpu, n)
        assert width >= 1 and c1_gpu.align_batch_width() == width
        got, _ = assert_batch_equals_singles(c1_gpu, guesses, 6, TSQ, 2.0, what=f"n {n}")   # forced rounds
        assert all(r.iterations == 6 for r in got)
        assert got.hypotheses_per_launch == width, n
        if width > 1:
            assert got.launches == -(-len(guesses) // width), n
        if n == widest_two:
            assert width == 2
        if n == widest_two + 1:
            assert width == 1
    assert c1_gpu.counter(1) == 0


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_a_batch_moves_nothing_else_and_forty_in_a_row_leave_nothing_behind(fan_ctx, fan_inputs):
    from eskf_lio_amd import synth
    vmap, pts, covs, guesses = fan_inputs
    before = fan_ctx.align_resident(guesses[1], 20, TSQ, COS)
    generation, size, exported = fan_ctx.counter(5), fan_ctx.map_size(), fan_ctx.map_export()
    fan_ctx.align_resident_batch(guesses, 20, TSQ, COS)
    after = fan_ctx.align_resident(guesses[1], 20, TSQ, COS)
    assert_same_bits(after, before, "single align around a batch")
    assert fan_ctx.counter(1) == 0 and fan_ctx.counter(5) == generation and fan_ctx.map_size() == size
    for a, b in zip(fan_ctx.map_export(), exported):
        assert a.tobytes() == b.tobytes()

    # forty batches on one context: k alternates, the resident scan alternates between two sizes (so the team size and
    # the owner of every exchange word change), converging and non-converging guesses mix, single aligns in between
    small = synth.make_structured_scan(20_000, vmap)[:2]
    scans = {27_000: (pts, covs), 20_000: small}
    pool = list(guesses) + jitter_guesses(5, seed=11)
    want = {}
    for n, (p, c) in scans.items():                          # the single calls' bits, once per scan and guess
        fan_ctx.scan_upload(p, c)
        want[n] = singles(fan_ctx, pool, 20, TSQ, COS)
    ks = (4, 2, 9, 3, 1, 5)
    for i in range(40):
        n = 27_000 if (i // 2) % 2 == 0 else 20_000
        if i % 2 == 0:
            fan_ctx.scan_upload(*scans[n])
        k = ks[i % len(ks)]
        pick = [(3 * i + 2 * j) % len(pool) for j in range(k)]
        if i % 3 == 0:
            pick[0] = 3                                      # the guess that does not converge
        got = fan_ctx.align_resident_batch([pool[j] for j in pick], 20, TSQ, COS)
        for h, j in enumerate(pick):
            assert_same_bits(got[h], want[n][j], f"batch {i} ({n} points, k {k}) hypothesis {h}")
        if i % 4 == 1:
            j = (5 * i) % len(pool)
            assert_same_bits(fan_ctx.align_resident(pool[j], 20, TSQ, COS), want[n][j], f"single align after batch {i}")
    assert fan_ctx.counter(1) == 0


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_batch_launch_that_gives_up_falls_back_once_and_cools_down(fan_inputs, monkeypatch):
    """A poll budget of zero: a bounded wait that runs out (in the field: another process holds compute units)."""
    from eskf_lio_amd import capi
    vmap, pts, covs, guesses = fan_inputs
    with capi.Context(0) as ref_ctx:
        load_map(ref_ctx, vmap)
        ref_ctx.scan_upload(pts, covs)
        want = singles(ref_ctx, guesses, 20, TSQ, COS)
    monkeypatch.setenv("VGICP_SPIN_LIMIT", "0")
    with capi.Context(0) as ctx:
        monkeypatch.delenv("VGICP_SPIN_LIMIT")
        load_map(ctx, vmap)
        ctx.scan_upload(pts, covs)
        assert ctx.align_batch_width() >= 2                  # 61 workgroups per team: room for two on 122 compute units
        for i in range(4):
            got = ctx.align_resident_batch(guesses, 20, TSQ, COS)
            for h in range(4):
                assert_same_bits(got[h], want[h], f"batch {i} hypothesis {h}")
            assert got.hypotheses_per_launch == 1 and got.launches > 4     # the launch-per-round loop
            # batch 0 attempts the launch and gives up: ONE fallback, not four.  Batches 1 and 2 are the eight aligns
            # of the cool-down: no launch, nothing counted.  Batch 3 tries again.
            assert (ctx.counter(0), ctx.counter(1)) == ((1, 1) if i < 3 else (2, 2)), i


# ---- 6 -------------------------------------------------------------------------------------------------------------
def test_paths_that_run_one_after_another(fan_inputs, c1_inputs):
    from eskf_lio_amd import capi, synth
    vmap, pts, covs, guesses = fan_inputs
    with capi.Context([0, 0]) as ctx:                        # a multi-device context
        load_map(ctx, vmap)
        ctx.scan_upload(pts, covs)
        got, _ = assert_batch_equals_singles(ctx, guesses[:3], 20, TSQ, COS, what="multi-device")
        assert got.hypotheses_per_launch == 1 and ctx.align_batch_width() == 1
    with capi.Context(0) as ctx:
        load_map(ctx, vmap)
        ctx.scan_upload(pts, covs)
        got, _ = assert_batch_equals_singles(ctx, guesses, 20, TSQ, COS, flags=capi.FLAG_NO_PERSISTENT,
                                             what="no persistent launch")
        assert got.hypotheses_per_launch == 1
        n = grid_of(ctx) * 448 + 1                           # several points per thread
        big = synth.make_uniform_scan(n, vmap)
        ctx.scan_upload(*big)
        got, _ = assert_batch_equals_singles(ctx, jitter_guesses(3), 4, TSQ, 2.0, what="several points per thread")
        assert got.hypotheses_per_launch == 1 and ctx.align_batch_width() == 1


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_a_member_without_correspondences_leaves_the_others_alone(fan_ctx, fan_inputs):
    _, _, _, guesses = fan_inputs
    far = guesses[0].copy()
    far[:3, 3] += 1.0e4                                      # every point lands outside the map (the K3 case)
    batch = [guesses[1], far, guesses[2]]
    got, want = assert_batch_equals_singles(fan_ctx, batch, 20, TSQ, COS, what="member without matches")
    assert got[1].corr_count[0] == 0 and got[1].status == want[1].status
    if fan_ctx.align_batch_width() >= 3:
        assert got.hypotheses_per_launch == 3 and got.launches == 1


# ---- 8 -------------------------------------------------------------------------------------------------------------
def test_a_pending_scan_is_settled_first(gpu_ctx, fan_inputs):
    from eskf_lio_amd import synth
    vmap, _, _, _ = fan_inputs
    load_map(gpu_ctx, vmap)
    raw = synth.make_lidar_scan(20_000, seed=3)
    guesses = jitter_guesses(3)
    kept, _ = gpu_ctx.scan_prepare(raw, None, None, None, vmap.voxel_size, 30)
    want = singles(gpu_ctx, guesses, 6, TSQ, 2.0)
    gpu_ctx.scan_prepare_async(raw, None, None, None, vmap.voxel_size, 30)
    got = gpu_ctx.align_resident_batch(guesses, 6, TSQ, 2.0)
    assert gpu_ctx.scan_info()[0] == kept
    for h in range(3):
        assert_same_bits(got[h], want[h], f"pending scan, hypothesis {h}")
    assert got.hypotheses_per_launch == min(3, max(expected_width(gpu_ctx, kept), 1))


# ---- 9 -------------------------------------------------------------------------------------------------------------
def select_best(converged, last_counts):
    """ICP::alignBest's rule: most correspondences in the last round, converged before unconverged, ties to the lower
    index."""
    best = 0
    for h in range(1, len(converged)):
        if (converged[h] and not converged[best]) or (converged[h] == converged[best] and
                                                       last_counts[h] > last_counts[best]):
            best = h
    return best


def test_shim_align_best_picks_what_the_rule_picks_from_the_oracle(fan_inputs, oracle):
    from eskf_lio_amd import host
    vmap, pts, covs, guesses = fan_inputs
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    refs = [om.align(pts, covs, g, 20, TSQ, COS) for g in guesses]
    want = select_best([r.converged for r in refs], [int(r.corr_count[-1]) for r in refs])
    assert want == 0 and want != 3                           # the counts of the issue's table; never the wrong basin
    lmap = host.LocalMap(vmap.voxel_size, 1)                 # one point per voxel: the voxel IS the mean + covariance
    lmap.updateLocalMap(vmap.means, vmap.covs, np.eye(4))
    assert len(lmap) == vmap.keys.shape[0]
    icp = host.ICP(20, TSQ, COS)
    pose = icp.alignBest(pts, covs, lmap, guesses)
    assert icp.best == want
    assert icp.converged == refs[want].converged and icp.iterations == refs[want].iterations
    dt, dr = pose_error(pose, refs[want].pose)
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and dt <= TIGHT_POSE_TOL and dr <= TIGHT_POSE_TOL
    # every hypothesis through alignHypotheses: the oracle's rounds, flags and last counts; the chosen pose's bits
    before = lmap.counter(2)
    hyps = icp.alignHypotheses(pts, covs, lmap, guesses)
    assert lmap.counter(2) - before == pts.shape[0] * 96 and not icp.used_resident     # ONE upload for four guesses
    assert len(hyps) == 4
    for h, ref in enumerate(refs):
        assert hyps[h]["iterations"] == ref.iterations and hyps[h]["converged"] == ref.converged
        assert hyps[h]["finalCorrespondences"] == int(ref.corr_count[-1])
        dt, dr = pose_error(hyps[h]["pose"], ref.pose)
        assert dt <= TIGHT_POSE_TOL and dr <= TIGHT_POSE_TOL
    assert np.array_equal(hyps[want]["pose"], pose)
    assert select_best([x["converged"] for x in hyps], [x["finalCorrespondences"] for x in hyps]) == want


def test_shim_hypotheses_on_a_stamped_cloud_do_not_upload():
    """CloudPreprocessor::process leaves the prepared scan resident and stamps the host cloud: alignHypotheses on that
    cloud registers the resident scan (VGICP_COUNTER_UPLOAD_BYTES does not move), with ICP::align's bits per guess."""
    from eskf_lio_amd import host, synth
    st = synth.make_imu_states(48, seed=9)
    n = 30_000
    t = synth.make_point_times(n, st[1, 0] + 1e-4, st[-3, 0] + 1e-3, seed=9)
    ext = synth.se3_to_SE3([0.01, -0.02, 0.03, 0.002, -0.001, 0.003])
    raws = [synth.make_lidar_scan(n, seed=60 + f) for f in range(2)]
    no_gate = dict(translation_sq_threshold=-1.0, cosine_threshold=2.0, remove_distant_points=False,
                   distance_threshold=1e9, removing_period=1e9, device_resident=True)
    fan = [synth.se3_to_SE3(xi) for xi in ([0.0] * 6, [0.02, -0.01, 0.0, 0.0, 0.0, 0.004], [-0.03, 0.02, 0.0, 0.0, 0.0, -0.006])]
    for host_copy in ("eager", "deferred"):
        pre = host.CloudPreprocessor(0.3, ext, host_copy)
        icp = host.ICP(12, TSQ, COS)
        lmap = host.LocalMap(0.3, 20, no_gate)
        first = host.Frame(raws[0], t, st)
        first.run(pre, icp, lmap, np.eye(4), first_frame=True)
        first.end()
        before = lmap.counter(2)
        fr = host.Frame(raws[1], t, st)
        hyps, used_resident, per_launch = fr.hypotheses(pre, icp, lmap, fan)
        assert used_resident and lmap.counter(2) == before, host_copy
        assert per_launch >= 1 and len(hyps) == 3
        fr.end()
        # the same cloud, as arrays, through plain ICP::align: one upload each, the same bits per guess
        gp, gc = host.CloudPreprocessor(0.3, ext, "eager").process(st, raws[1], t)
        for h, g in enumerate(fan):
            single = host.ICP(12, TSQ, COS)
            pose = single.align(gp, gc, lmap, g)
            assert np.array_equal(hyps[h]["pose"], pose), (host_copy, h)
            assert hyps[h]["iterations"] == single.iterations and hyps[h]["converged"] == single.converged
            assert hyps[h]["finalCorrespondences"] == int(single.correspondence_counts[-1])
        assert lmap.counter(2) > before
