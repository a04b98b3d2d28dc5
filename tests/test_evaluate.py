"""vgicp_evaluate_resident (include/vgicp_hip_evaluate.h): the resident scan scored at several poses in one launch pair —
correspondences, the VGICP objective, the squared error and the normal equations at each pose.

Counts are held against the CPU oracle exactly, cost and sq_error within bounds derived below (not fitted); the normal
equations and counts are bit for bit what the existing paths produce for round 0 from the same pose, so every such
comparison is `==` / np.array_equal.
"""
import ctypes as C
import math

import numpy as np
import pytest

from test_align_batch import FAN_XI, COS, TSQ, grid_of, jitter_guesses, load_map

pytestmark = pytest.mark.gpu

U = 2.0 ** -53                      # unit roundoff of fp64
MISS_PENALTY = 11.345               # ICP::Evaluation::score's default: the 0.99 quantile of chi-squared, 3 degrees of freedom
# first-order operation count of one cost term (derivation: test_counts_cost_and_error_against_the_oracle's docstring)
COST_C = 72


@pytest.fixture(scope="module")
def fan_inputs():
    from eskf_lio_amd import synth
    vmap = synth.make_map(50_000)
    pts, covs, _ = synth.make_structured_scan(27_000, vmap)
    return vmap, pts, covs, [synth.se3_to_SE3(xi) for xi in FAN_XI]


@pytest.fixture(scope="module")
def fan_oracle(fan_inputs, oracle):
    """The oracle's map, and its four returned poses for the fan."""
    vmap, pts, covs, guesses = fan_inputs
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    refs = [om.align(pts, covs, g, 20, TSQ, COS) for g in guesses]
    return om, refs


@pytest.fixture()
def fan_ctx(gpu_ctx, fan_inputs):
    vmap, pts, covs, _ = fan_inputs
    load_map(gpu_ctx, vmap)
    gpu_ctx.scan_upload(pts, covs)
    return gpu_ctx


def exact_sum(terms_ld):
    """The sum of extended-precision terms, rounded once: every term split into two doubles, added by math.fsum."""
    hi = terms_ld.astype(np.float64)
    lo = (terms_ld - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(list(hi) + list(lo))


def reference_sums(oracle, om, pts, covs, pose):
    """(count, cost, sq_error, largest condition number) at `pose` from the oracle's transform and match.  The terms
    are formed in extended precision (64-bit significand), so the reference's own error is 2^-11 of fp64's."""
    tp, tc = oracle.transform(pts, covs, pose)
    sp, sc, mp, mc, _ = om.match(tp, tc)
    m = sp.shape[0]
    if m == 0:
        return 0, 0.0, 0.0, 1.0
    S64 = (sc + mc).reshape(m, 3, 3)
    kappa = float(np.linalg.cond(S64).max())
    S = sc.astype(np.longdouble).reshape(m, 3, 3) + mc.astype(np.longdouble).reshape(m, 3, 3)
    e = sp.astype(np.longdouble) - mp.astype(np.longdouble)
    # x = S^-1 e by Cramer's rule in extended precision
    det = (S[:, 0, 0] * (S[:, 1, 1] * S[:, 2, 2] - S[:, 1, 2] * S[:, 2, 1])
           - S[:, 0, 1] * (S[:, 1, 0] * S[:, 2, 2] - S[:, 1, 2] * S[:, 2, 0])
           + S[:, 0, 2] * (S[:, 1, 0] * S[:, 2, 1] - S[:, 1, 1] * S[:, 2, 0]))
    adj = np.empty_like(S)
    for r in range(3):
        for c in range(3):
            r0, r1 = [k for k in range(3) if k != c]      # adj[r][c] = cofactor[c][r]
            c0, c1 = [k for k in range(3) if k != r]
            adj[:, r, c] = (-1) ** (r + c) * (S[:, r0, c0] * S[:, r1, c1] - S[:, r0, c1] * S[:, r1, c0])
    x = np.einsum("mrc,mc->mr", adj, e) / det[:, None]
    cost = exact_sum(np.einsum("mr,mr->m", e, x))
    sq = exact_sum(np.einsum("mr,mr->m", e, e))
    return m, cost, sq, kappa


def same_evaluation(a, b):
    return (a.points == b.points and a.correspondences == b.correspondences and
            np.array([a.cost, a.sq_error]).tobytes() == np.array([b.cost, b.sq_error]).tobytes() and
            a.normal_eq.tobytes() == b.normal_eq.tobytes())


def row0(ctx, pose, flags=0):
    """Round 0 of an align from `pose`: (count, 27 normal equations)."""
    r = ctx.align_resident(pose, 1, TSQ, 2.0, flags=flags, allow_degenerate=True)
    assert r.iterations == 1
    return int(r.corr_count[0]), r.normal_eq[0]


def packed(JTJ, JTr):
    return np.array([JTJ[r, c] for r in range(6) for c in range(r + 1)] + list(JTr))


# ---- 1, 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_counts_cost_and_error_against_the_oracle(fan_ctx, fan_inputs, fan_oracle, oracle):
    """The four guesses of the fan and the oracle's four returned poses: `correspondences` equals the oracle's match
    count exactly; cost and sq_error are held against the same sums formed from the oracle's matched arrays.

    Bounds (u = 2^-53, m = correspondences, every term non-negative, so bounds relative to the sum carry over from the
    terms):
      sq_error  two orders of summing m non-negative terms differ by at most 2 (m - 1) u, plus 4 u for each term's own
                rounding under contraction: (2 (m - 1) + 4) u.
      cost      the same, plus the cofactor inverse and the quadratic form, c kappa^2 u with kappa the largest 2-norm
                condition number of S = src_cov + map_cov over the matched pairs (measured below) and c = 72, counted to
                first order with |S_ij| <= ||S|| = l1 >= l2 >= l3 > 0 the eigenvalues:
                  13  S itself: the kernel forms R C R^T with contraction, the oracle without — two 3-term dot
                      products each (6 u against the exact value, twice) and the one addition of C_voxel; a
                      perturbation dS of S moves e^T S^-1 e by at most kappa ||dS|| / ||S|| relative (<= kappa^2)
                  27  det: a cofactor a b - c d as one multiply and one fma is off by <= 3 u ||S||^2; three of them times
                      an entry: 9 u ||S||^3; the 3-term dot product itself: 3 u times sum |c_i S_i| <= 6 ||S||^3: 18 u
                      ||S||^3; relative to det = l1 l2 l3 that is 27 u l1^2 / (l2 l3) <= 27 kappa^2 u
                   2  the reciprocal (v_rcp_f64 + one third-order step, ~1 ulp)
                   9  the adjugate in the numerator e^T adj(S) e = cost x det >= |e|^2 l2 l3: nine entries off by
                      <= 3 u ||S||^2 against (sum |e_i|)^2 <= 3 |e|^2: 9 u l1^2 / (l2 l3)
                  21  scaling by 1 / det (1), W e (3) and e . (W e) (3): 7 roundings, each relative to sum |e_i| |W_ij|
                      |e_j| <= 3 |e|^2 / l3 against cost >= |e|^2 / l1: 21 kappa u <= 21 kappa^2 u
    Observed on an MI355X (largest relative difference over the 8 poses): cost 2.1e-16, sq_error 1.2e-16, against bounds
    of 8.2e-11 - 8.6e-11 and 2.6e-12 - 6.0e-12 (Scoring a pose)."""
    vmap, pts, covs, guesses = fan_inputs
    om, refs = fan_oracle
    poses = list(guesses) + [r.pose for r in refs]
    got = fan_ctx.evaluate_resident(poses)
    assert len(got) == 8 and got.launches == 2 and got.poses_per_launch >= 16
    counts, worst_cost, worst_sq = [], 0.0, 0.0
    for h, pose in enumerate(poses):
        m, cost, sq, kappa = reference_sums(oracle, om, pts, covs, pose)
        counts.append(m)
        g = got[h]
        assert g.points == pts.shape[0] and g.correspondences == m, (h, g.correspondences, m)
        assert m > 0
        sq_bound = (2 * (m - 1) + 4) * U
        cost_bound = sq_bound + COST_C * kappa * kappa * U
        d_sq, d_cost = abs(g.sq_error - sq) / sq, abs(g.cost - cost) / cost
        print(f"pose {h}: m {m} kappa {kappa:.1f} cost {g.cost!r} ref {cost!r} rel {d_cost:.3e} (bound {cost_bound:.3e}) "
              f"sq_error {g.sq_error!r} ref {sq!r} rel {d_sq:.3e} (bound {sq_bound:.3e})")
        worst_cost, worst_sq = max(worst_cost, d_cost), max(worst_sq, d_sq)
        assert d_sq <= sq_bound, (h, d_sq, sq_bound)
        assert d_cost <= cost_bound, (h, d_cost, cost_bound)
        assert g.fitness == m / pts.shape[0] and g.inlier_rmse == float(np.sqrt(g.sq_error / m))
    print(f"counts {counts}; largest relative difference: cost {worst_cost:.3e}, sq_error {worst_sq:.3e}")
    # what the feature is for: the returned poses of the right basin match every point, the wrong basin's does not, and
    # the last-round count an align reports is not the count of the pose it returns
    assert counts[4:7] == [pts.shape[0]] * 3 and counts[7] < pts.shape[0] // 2
    assert any(int(r.corr_count[-1]) != counts[4 + h] for h, r in enumerate(refs))


# ---- 3 -------------------------------------------------------------------------------------------------------------
SIZES = [1, 447, 448, 449, 27_000, 256 * 448, 256 * 448 + 1, 200_000]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("symmetric", [True, False], ids=["nine-planes", "twelve-planes"])
def test_normal_equations_are_round_zero_of_every_existing_path(c1_gpu, c1_inputs, symmetric):
    from eskf_lio_amd import capi, synth
    vmap, _, _ = c1_inputs
    poses = jitter_guesses(3)
    grid = grid_of(c1_gpu)
    with capi.Context(0) as other:                           # vgicp_accumulate replaces the resident scan: a second context
        load_map(other, vmap)
        for n in SIZES:
            pts, covs = synth.make_uniform_scan(n, vmap)
            if not symmetric:
                covs = covs.copy()
                covs[:, 1] += 1e-7                           # c10 != c01: all twelve planes are read
            c1_gpu.scan_upload(pts, covs)
            got = c1_gpu.evaluate_resident(poses)
            assert got.poses_per_launch >= (16 if n <= 256 * 448 else 8), n
            for h, pose in enumerate(poses):
                what = f"n {n} pose {h}"
                assert got[h].points == n
                count, neq = row0(c1_gpu, pose, capi.FLAG_NO_PERSISTENT)
                assert got[h].correspondences == count and np.array_equal(got[h].normal_eq, neq), what + " (loop)"
                if n <= grid * 448:
                    count, neq = row0(c1_gpu, pose)
                    assert got[h].correspondences == count and np.array_equal(got[h].normal_eq, neq), what + " (persistent)"
                JTJ, JTr, count = other.accumulate(pts, covs, pose)
                assert got[h].correspondences == count and np.array_equal(got[h].normal_eq, packed(JTJ, JTr)), what + " (accumulate)"
                assert np.array_equal(got[h].JTJ, JTJ) and np.array_equal(got[h].JTr, JTr)
    assert c1_gpu.counter(1) == 0


# ---- 4 -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", [27_000, 120_000])             # one launch pair for 64 poses; 15 poses per launch pair
def test_a_pose_does_not_depend_on_k_position_or_neighbours(c1_gpu, c1_inputs, n):
    from eskf_lio_amd import synth
    vmap, _, _ = c1_inputs
    pts, covs = synth.make_uniform_scan(n, vmap)
    c1_gpu.scan_upload(pts, covs)
    probe = synth.default_guess()
    fill = jitter_guesses(64, seed=7)
    other_fill = jitter_guesses(64, seed=8)
    want = c1_gpu.evaluate_resident([probe])
    assert len(want) == 1 and want.launches == 2
    assert want[0].correspondences > 0 and want[0].cost > 0.0 and want[0].sq_error > 0.0
    per_launch = want.poses_per_launch
    assert per_launch == min(64, 4096 // -(-n // 448))
    for k in (1, 4, 16, 17, 64):
        for neighbours in (fill, other_fill):
            for pos in sorted({0, k // 2, k - 1}):
                batch = [neighbours[i] for i in range(k)]
                batch[pos] = probe
                got = c1_gpu.evaluate_resident(batch)
                assert len(got) == k and got.launches == 2 * -(-k // per_launch)
                assert same_evaluation(got[pos], want[0]), (k, pos)
    batch = fill[:17]
    a, b = c1_gpu.evaluate_resident(batch), c1_gpu.evaluate_resident(batch)
    assert all(same_evaluation(x, y) for x, y in zip(a, b))
    assert not same_evaluation(a[0], a[1])                   # different poses do differ


# ---- 5 -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_an_evaluation_changes_nothing(fan_inputs):
    from eskf_lio_amd import capi
    from test_align_batch import assert_same_bits
    vmap, pts, covs, guesses = fan_inputs

    def calls(ctx):
        return (ctx.align_resident(guesses[1], 20, TSQ, COS),
                ctx.align_resident_batch(guesses, 20, TSQ, COS),
                ctx.align_resident(guesses[2], 20, TSQ, COS, flags=capi.FLAG_NO_PERSISTENT),
                ctx.align_resident(guesses[0], 20, TSQ, COS))

    with capi.Context(0) as fresh:                           # never evaluates
        load_map(fresh, vmap)
        fresh.scan_upload(pts, covs)
        want = calls(fresh)
    with capi.Context(0) as ctx:
        load_map(ctx, vmap)
        ctx.scan_upload(pts, covs)
        info, generation = ctx.scan_info(), ctx.counter(5)
        exported, scan = ctx.map_export(), ctx.scan_download()
        first = ctx.evaluate_resident(guesses)
        got = calls(ctx)
        for g, w, what in zip(got, want, ("align", "batch", "loop align", "second align")):
            if what == "batch":
                for h in range(len(guesses)):
                    assert_same_bits(g[h], w[h], f"batch hypothesis {h} after an evaluation")
            else:
                assert_same_bits(g, w, what + " after an evaluation")
        # ... and in between the calls, in a different order
        ctx.evaluate_resident(guesses[:1])
        assert_same_bits(ctx.align_resident_batch(guesses, 20, TSQ, COS)[3], want[1][3], "batch, again")
        ctx.evaluate_resident(guesses * 5)
        assert_same_bits(ctx.align_resident(guesses[1], 20, TSQ, COS), want[0], "align, again")
        again = ctx.evaluate_resident(guesses)
        assert all(same_evaluation(a, b) for a, b in zip(first, again))
        assert ctx.scan_info() == info and ctx.counter(5) == generation and ctx.counter(1) == 0
        for a, b in zip(ctx.map_export(), exported):
            assert a.tobytes() == b.tobytes()
        for a, b in zip(ctx.scan_download(), scan):
            assert a.tobytes() == b.tobytes()


# ---- 6 -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_sixteen_poses_cost_one_synchronisation_and_two_launches(fan_ctx):
    poses = jitter_guesses(16)
    fan_ctx.evaluate_resident(poses)
    fan_ctx.frame_stats(reset=True)
    got = fan_ctx.evaluate_resident(poses)
    fs = fan_ctx.frame_stats()
    assert fs.host_syncs == 1 and fs.kernel_launches <= 2 and fs.copies == 0
    assert got.poses_per_launch >= 16 and got.launches == 2
    assert got.seconds > 0.0 and got.device_seconds > 0.0


# ---- 7 -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_edges(fan_ctx, fan_inputs):
    from eskf_lio_amd import capi, synth
    vmap, pts, covs, guesses = fan_inputs
    lib = capi.load_library()
    far = guesses[0].copy()
    far[:3, 3] += 1.0e4                                      # every point lands outside the map
    got = fan_ctx.evaluate_resident([guesses[0], far, guesses[1]])
    e = got[1]
    assert e.points == pts.shape[0] and e.correspondences == 0 and e.fitness == 0.0 and e.inlier_rmse == 0.0
    zeros = np.zeros(29)
    assert np.concatenate([[e.cost, e.sq_error], e.normal_eq]).tobytes() == zeros.tobytes()      # +0.0, every one
    assert same_evaluation(got[0], fan_ctx.evaluate_resident([guesses[0]])[0])
    # the range of k, NULL pointers, a pose that is not finite: refused on the host, `out` untouched
    out = (capi.Evaluation * 65)()
    C.memset(out, 0xA5, C.sizeof(out))
    before = bytes(out)
    g = np.ascontiguousarray(np.stack([capi.pose_to_abi(guesses[h % 4]) for h in range(65)]))
    dp = g.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.vgicp_evaluate_resident(fan_ctx._h, 0, dp, out, None) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_evaluate_resident(fan_ctx._h, 65, dp, out, None) == capi.ERR_BAD_ARGUMENT
    assert "VGICP_EVAL_MAX" in fan_ctx.last_error()
    assert lib.vgicp_evaluate_resident(fan_ctx._h, 4, None, out, None) == capi.ERR_BAD_ARGUMENT
    assert lib.vgicp_evaluate_resident(fan_ctx._h, 4, dp, None, None) == capi.ERR_BAD_ARGUMENT
    for bad in (np.nan, np.inf):
        g[3, 13] = bad                                       # pose 3 of 4
        assert lib.vgicp_evaluate_resident(fan_ctx._h, 4, dp, out, None) == capi.ERR_BAD_ARGUMENT
        assert "pose 3" in fan_ctx.last_error()
    assert bytes(out) == before
    g[3, 13] = 0.0
    assert lib.vgicp_evaluate_resident(fan_ctx._h, 64, dp, out, None) == capi.OK
    assert bytes(out)[:64 * 248] != before[:64 * 248] and bytes(out)[64 * 248:] == before[64 * 248:]
    # no map, no scan
    with capi.Context(0) as ctx:
        with pytest.raises(capi.VgicpError) as err:
            ctx.evaluate_resident(guesses)
        assert err.value.code == capi.ERR_NOT_READY
        load_map(ctx, vmap)
        with pytest.raises(capi.VgicpError) as err:
            ctx.evaluate_resident(guesses)
        assert err.value.code == capi.ERR_NOT_READY
        # a scan that is still pending is settled and evaluated
        raw = synth.make_lidar_scan(20_000, seed=3)
        kept, _ = ctx.scan_prepare(raw, None, None, None, vmap.voxel_size, 30)
        want = ctx.evaluate_resident(guesses[:3])
        ctx.scan_prepare_async(raw, None, None, None, vmap.voxel_size, 30)
        pending = ctx.evaluate_resident(guesses[:3])
        assert ctx.scan_info()[0] == kept and all(p.points == kept for p in pending)
        assert all(same_evaluation(a, b) for a, b in zip(pending, want))
    # a multi-device context shards the scan: refused, with a text
    with capi.Context([0, 0]) as multi:
        load_map(multi, vmap)
        multi.scan_upload(pts, covs)
        with pytest.raises(capi.VgicpError) as err:
            multi.evaluate_resident(guesses)
        assert err.value.code == capi.ERR_BAD_ARGUMENT and "not available on multi-device contexts" in str(err.value)


# ---- 8 -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_shim_align_best_by_score(fan_inputs, fan_oracle, oracle):
    from eskf_lio_amd import capi, host
    vmap, pts, covs, guesses = fan_inputs
    om, refs = fan_oracle
    # the rule on the oracle's returned poses, in numpy: converged first, then the lowest score, ties to the lower index
    scores, kappa = [], 1.0
    for r in refs:
        m, cost, _, k = reference_sums(oracle, om, pts, covs, r.pose)
        scores.append(cost + MISS_PENALTY * (pts.shape[0] - m))
        kappa = max(kappa, k)
    order = sorted(range(4), key=lambda h: (not refs[h].converged, scores[h], h))
    want = order[0]
    assert want in (0, 1, 2) and order[-1] == 3              # the wrong basin comes last

    lmap = host.LocalMap(vmap.voxel_size, 1)                 # one point per voxel: the voxel IS the mean + covariance
    lmap.updateLocalMap(vmap.means, vmap.covs, np.eye(4))
    icp = host.ICP(20, TSQ, COS)
    pose = icp.alignBestByScore(pts, covs, lmap, guesses)
    assert icp.best in (0, 1, 2) and icp.converged == refs[icp.best].converged and icp.iterations == refs[icp.best].iterations
    # the same choice as the oracle's scores make — unless the oracle's own best two are closer than the bound on a cost
    gap = (scores[order[1]] - scores[want]) / scores[want]
    near = (2 * pts.shape[0] + COST_C * kappa ** 2) * U
    print(f"oracle scores {scores}, chosen {icp.best}, wanted {want}, relative gap to the runner-up {gap:.3e}")
    if gap > near:
        assert icp.best == want
    else:
        assert abs(scores[icp.best] - scores[want]) / scores[want] <= near
    hyps = icp.alignHypotheses(pts, covs, lmap, guesses)
    assert np.array_equal(hyps[icp.best]["pose"], pose)
    ev = icp.evaluation
    assert ev.points == pts.shape[0] and ev.correspondences == pts.shape[0] and ev.fitness == 1.0
    # lastEvaluation() is the evaluation of that pose: through the shim on the same map, and through the C ABI on a
    # context that holds the same voxels
    again = icp.evaluate(pts, covs, lmap, [pose, guesses[3]])
    assert not icp.used_resident and same_evaluation(again[0], ev) and again[1].correspondences < pts.shape[0] // 2
    keys, means, vcovs, _ = lmap.export()
    with capi.Context(0) as ctx:
        ctx.map_reset(vmap.voxel_size, keys.shape[0])
        ctx.map_upsert(keys, means, vcovs)
        ctx.scan_upload(pts, covs)
        direct = ctx.evaluate_resident([pose])[0]
    assert same_evaluation(direct, ev)


@pytest.mark.timeout(600)
def test_shim_evaluate_reads_the_resident_scan_or_the_cloud_as_it_is_now():
    """CloudPreprocessor::process leaves the prepared scan resident and stamps the host cloud: ICP::evaluate on that
    cloud reads the resident scan (no upload); after an in-place edit or a resize it uploads the cloud as it is now."""
    from eskf_lio_amd import host, synth
    st = synth.make_imu_states(48, seed=9)
    n = 30_000
    t = synth.make_point_times(n, st[1, 0] + 1e-4, st[-3, 0] + 1e-3, seed=9)
    ext = synth.se3_to_SE3([0.01, -0.02, 0.03, 0.002, -0.001, 0.003])
    raws = [synth.make_lidar_scan(n, seed=60 + f) for f in range(2)]
    no_gate = dict(translation_sq_threshold=-1.0, cosine_threshold=2.0, remove_distant_points=False,
                   distance_threshold=1e9, removing_period=1e9, device_resident=True)
    poses = [np.eye(4), synth.se3_to_SE3([0.02, -0.01, 0.0, 0.0, 0.0, 0.004])]
    for host_copy in ("eager", "deferred"):
        pre = host.CloudPreprocessor(0.3, ext, host_copy)
        icp = host.ICP(12, TSQ, COS)
        lmap = host.LocalMap(0.3, 20, no_gate)
        first = host.Frame(raws[0], t, st)
        first.run(pre, icp, lmap, np.eye(4), first_frame=True)
        first.end()
        results = {}
        for mutate in (0, 1, 2):
            before = lmap.counter(2)
            fr = host.Frame(raws[1], t, st)
            evs, used_resident = fr.evaluate(pre, icp, lmap, poses, mutate=mutate)
            fr.end()
            assert used_resident == (mutate == 0), (host_copy, mutate)
            assert (lmap.counter(2) == before) == (mutate == 0)          # VGICP_COUNTER_UPLOAD_BYTES
            results[mutate] = evs
        # the same cloud as arrays: one upload, the resident scan's bits
        gp, gc = host.CloudPreprocessor(0.3, ext, "eager").process(st, raws[1], t)
        arrays = icp.evaluate(gp, gc, lmap, poses)
        kept = gp.shape[0]
        for h in range(2):
            assert results[0][h].points == kept and results[0][h].correspondences > 0
            assert same_evaluation(results[0][h], arrays[h]), (host_copy, h)
            assert results[2][h].points == kept - 1                      # the resized cloud is what was evaluated
            assert results[1][h].points == kept
        gp1 = gp.copy()
        gp1[0, 0] += 1e-3                                                # the edit host_frame_evaluate makes
        edited = icp.evaluate(gp1, gc, lmap, poses)
        assert all(same_evaluation(results[1][h], edited[h]) for h in range(2))
