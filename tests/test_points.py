"""vgicp_points_resident (include/vgicp_hip_points.h): the resident scan at a pose, point by point — matched or not,
raw d^2, |e|^2, the weight under the context's robust options — and order statistics of d^2.

The reference is tests/points_reference.py (the oracle's transform and match, d^2 in extended precision, the header's
weights), whose preconditions tests/test_points_cpu.py checks.  The scene is tests/test_robust.py's.  Bounds are derived
(u = 2^-53, kappa measured in the test), never fitted; everything that compares two device results is bit for bit.
"""
import ctypes as C
import math

import numpy as np
import pytest

import points_reference as pr
import robust_reference as rr
from points_reference import GATES, MATCHED, NEGATIVE, NOT_FINITE, QS, U
from test_align_batch import assert_same_bits, jitter_guesses, load_map
from test_evaluate import COST_C

pytestmark = pytest.mark.gpu

COUNTER_FALLBACKS, COUNTER_SCAN_GENERATION = 1, 5
SIZES = [1, 63, 64, 65, 255, 256, 257, 1024, 1025, 6000]
TSQ = 1e-12
assert COST_C == pr.COST_C


@pytest.fixture(scope="module")
def scene(oracle):
    vmap, pts, covs, T_true, guess = rr.make_scene()
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    return vmap, om, pts, covs, T_true, guess


@pytest.fixture(scope="module")
def references(scene, oracle):
    """The reference at T_true and at the guess, computed once."""
    _, om, pts, covs, T_true, guess = scene
    return {"T_true": pr.reference_at(oracle, om, pts, covs, T_true), "guess": pr.reference_at(oracle, om, pts, covs, guess)}


@pytest.fixture()
def scene_ctx(gpu_ctx, scene):
    vmap, _, pts, covs, _, _ = scene
    load_map(gpu_ctx, vmap)
    gpu_ctx.scan_upload(pts, covs)
    return gpu_ctx


def pose_of(scene, where):
    return scene[4] if where == "T_true" else scene[5]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_report(a, b, n=None):
    cut = (lambda x: x) if n is None else (lambda x: x[:n])
    return all(same_bits(cut(x), y) for x, y in ((a.d2, b.d2), (a.sq_error, b.sq_error), (a.weight, b.weight),
                                                 (a.status, b.status)))


def term_bound(kappa):
    return COST_C * kappa * kappa * U


def check_quantiles(ctx, pose, rep, ref):
    """Item 2 for the report `rep` (all arrays, quantiles QS) of the scan that is resident: each quantile is, bit for
    bit, the element of its rank of the returned d2 array itself; within the term bound of the reference's order
    statistic; and the same bits come back without the per-point arrays."""
    ranked_mask = (rep.status & MATCHED != 0) & (rep.status & NOT_FINITE == 0)
    own = np.sort(np.maximum(rep.d2[ranked_mask], 0.0))
    want = pr.order_statistics(own, QS)
    assert same_bits(rep.quantiles, want) or (len(own) == 0 and np.isnan(rep.quantiles).all()), (rep.quantiles, want)
    theirs = pr.order_statistics(ref.ranked, QS)
    assert len(own) == len(ref.ranked)
    if len(own):
        worst = float(np.max(np.abs(rep.quantiles - theirs) / theirs))
        assert worst <= term_bound(ref.kappa), (worst, rep.quantiles, theirs)
    alone = ctx.points_resident(pose, QS, d2=False, sq_error=False, weight=False, status=False)
    assert alone.d2 is None and alone.status is None and same_bits(alone.quantiles, rep.quantiles)
    assert (alone.matched, alone.counted, alone.negative, alone.not_finite) == \
        (rep.matched, rep.counted, rep.negative, rep.not_finite)
    return rep.quantiles


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["T_true", "guess"])
def test_points_against_the_reference(scene_ctx, scene, references, where):
    """MATCHED is exactly the oracle's matched index set; every matched d2 within COST_C kappa^2 u (relative) of
    rr.mahalanobis_sq — the bound of one cost term, derived in tests/test_evaluate.py — and sq_error within 8 u: three
    subtractions (1 u each, doubled by the square), three products and two additions under contraction; unmatched
    entries are +inf, +inf, 0 and 0; the counts are the reference's.  Weights, for the four modes of rr.MODES, within
    (COST_C kappa^2 + 16) u of rr.weights: for Huber and Cauchy |dw / w| <= |dd^2 / d^2| (w = c / d and w = c^2 / (c^2 +
    d^2)) and w <= 1, the 16 u cover v_rsq_f64 / rcp_newton with their third-order steps and the products around them;
    with the defaults every matched weight is exactly 1.0.

    Observed on an MI355X (worst over both poses): d2 1.4e-14 relative against a bound of 8.0e-11, sq_error 2.7e-16
    against 8.9e-16, weights 3.1e-15 (Cauchy), 5.2e-15 (Huber), 0 (gate), 2.7e-15 (Cauchy + gate) against 8.0e-11
    (Per-point terms)."""
    pose, ref = pose_of(scene, where), references[where]
    n = ref.n
    rep = scene_ctx.points_resident(pose)
    assert rep.points == n == 6000 and rep.launches == 2 and len(rep.quantiles) == 0
    want_d2, want_sq, want_w, want_status = ref.planes()
    assert np.array_equal(np.flatnonzero(rep.status & MATCHED), ref.index)
    assert np.array_equal(rep.status, want_status)
    miss = rep.status == 0
    assert np.all(np.isposinf(rep.d2[miss])) and np.all(np.isposinf(rep.sq_error[miss])) and not rep.weight[miss].any()
    assert miss.sum() == n - len(ref.index) > 0
    hit = ~miss
    d_d2 = float(np.max(np.abs(rep.d2[hit] - ref.raw) / np.abs(ref.raw)))
    d_sq = float(np.max(np.abs(rep.sq_error[hit] - ref.sq) / ref.sq))
    bound = term_bound(ref.kappa)
    print(f"{where}: matched {rep.matched} kappa {ref.kappa:.4f}; worst relative difference d2 {d_d2:.3e} (bound {bound:.3e}) "
          f"sq_error {d_sq:.3e} (bound {8 * U:.3e})")
    assert d_d2 <= bound and d_sq <= 8 * U
    assert (rep.matched, rep.negative, rep.not_finite) == (len(ref.index), 0, 0)
    assert rep.counted == rep.matched and np.all(rep.weight[hit] == 1.0)        # the defaults
    for mode, (kernel, c, gate) in rr.MODES.items():
        scene_ctx.set_robust(kernel, c, gate)
        got = scene_ctx.points_resident(pose)
        want = ref.planes(kernel, c, gate)[2]
        d_w = float(np.max(np.abs(got.weight - want)))
        print(f"{where} / {mode}: worst weight difference {d_w:.3e} (bound {bound + 16 * U:.3e}), counted {got.counted}")
        assert d_w <= bound + 16 * U
        assert np.array_equal(got.weight > 0.0, want > 0.0) and got.counted == int(np.count_nonzero(want > 0.0))
        assert same_bits(got.d2, rep.d2) and same_bits(got.sq_error, rep.sq_error) and same_bits(got.status, rep.status)
    scene_ctx.set_robust("none", 1.0, 0.0)
    assert same_report(scene_ctx.points_resident(pose), rep)


# ---- 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["T_true", "guess"])
def test_quantiles_are_order_statistics_of_the_returned_array(scene_ctx, scene, references, where):
    pose, ref = pose_of(scene, where), references[where]
    rep = scene_ctx.points_resident(pose, QS)
    assert rep.launches == 2 + 1 + 3                  # 6000 pairs are 24 tiles: the tile sort and three merge levels
    q = check_quantiles(scene_ctx, pose, rep, ref)
    print(f"{where}: quantiles {QS} of d^2: {q}")
    assert same_report(rep, scene_ctx.points_resident(pose))      # the arrays do not depend on the quantiles
    assert q[0] == rep.d2.min() and q[-1] == rep.d2[np.isfinite(rep.d2)].max() and np.all(np.diff(q) >= 0)


# ---- 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["T_true", "guess"])
def test_agreement_with_the_paths_that_exist(scene_ctx, scene, references, where):
    """The sums of the arrays against vgicp_evaluate_resident (two orders of summing m non-negative terms: (2 (m - 1) +
    4) u, and the term bound for cost, whose terms the evaluation forms beside the normal equations), and `counted`
    against the robust round's own count: for each gate, with kernel none, counted == count_nonzero(d2 <= g) ==
    corr_count[0] of a one-round robust align from that pose, the persistent launch and the loop alike.

    Observed on an MI355X: the sum of d2 equals the evaluation's cost (difference 0 at both poses), the sum of sq_error
    its squared error to 1.2e-16."""
    from eskf_lio_amd import capi
    pose, ref = pose_of(scene, where), references[where]
    rep = scene_ctx.points_resident(pose)
    ev = scene_ctx.evaluate_resident([pose])[0]
    hit = rep.status & MATCHED != 0
    m = int(hit.sum())
    assert rep.matched == ev.correspondences == m
    sum_bound = (2 * (m - 1) + 4) * U
    d_cost = abs(math.fsum(rep.d2[hit]) - ev.cost) / ev.cost
    d_sq = abs(math.fsum(rep.sq_error[hit]) - ev.sq_error) / ev.sq_error
    print(f"{where}: cost {d_cost:.3e} (bound {sum_bound + term_bound(ref.kappa):.3e}) sq_error {d_sq:.3e} (bound {sum_bound:.3e})")
    assert d_cost <= sum_bound + term_bound(ref.kappa) and d_sq <= sum_bound
    for gate in GATES:
        scene_ctx.set_robust("none", 1.0, gate)
        gated = scene_ctx.points_resident(pose)
        inside = int(np.count_nonzero(rep.d2 <= gate))
        assert gated.counted == inside == int(np.count_nonzero(gated.weight > 0.0)) == int(np.count_nonzero(ref.raw <= gate))
        assert 0 < inside < m
        for flags in (0, capi.FLAG_NO_PERSISTENT):
            r = scene_ctx.align_resident(pose, 1, TSQ, 2.0, flags=flags, allow_degenerate=True)
            assert r.iterations == 1 and int(r.corr_count[0]) == inside, (gate, flags, r.corr_count, inside)
    assert scene_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_sizes_and_independence(gpu_ctx, scene, references):
    """Prefixes of the scan over the wave, tile and block edges of the kernel (64, 256) and of the sort (256-pair tiles,
    merges of 2 and 4 runs): each call's arrays are the first n entries of the whole scan's, twice the same, one array
    at a time the same, and the quantiles are the order statistics of the prefix."""
    vmap, _, pts, covs, T_true, _ = scene
    load_map(gpu_ctx, vmap)
    gpu_ctx.set_robust("cauchy", 0.15, 0.06)                  # weights that differ from point to point
    gpu_ctx.scan_upload(pts, covs)
    whole = gpu_ctx.points_resident(T_true, QS)
    assert whole.points == 6000
    for n in SIZES:
        gpu_ctx.scan_upload(pts[:n], covs[:n])
        rep = gpu_ctx.points_resident(T_true, QS)
        assert rep.points == n and all(len(a) == n for a in (rep.d2, rep.sq_error, rep.weight, rep.status))
        assert same_report(whole, rep, n), n
        again = gpu_ctx.points_resident(T_true, QS)
        assert same_report(again, rep) and same_bits(again.quantiles, rep.quantiles), n
        for name in ("d2", "sq_error", "weight", "status"):
            one = gpu_ctx.points_resident(T_true, **{k: k == name for k in ("d2", "sq_error", "weight", "status")})
            assert same_bits(getattr(one, name), getattr(rep, name)), (n, name)
            assert sum(getattr(one, k) is not None for k in ("d2", "sq_error", "weight", "status")) == 1
            assert (one.matched, one.counted) == (rep.matched, rep.counted)
        check_quantiles(gpu_ctx, T_true, rep, references["T_true"].prefix(n))
        assert rep.matched == int(np.count_nonzero(rep.status & MATCHED))
        assert rep.counted == int(np.count_nonzero(rep.weight > 0.0))


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_nothing_matched(scene_ctx, scene):
    far = np.array(scene[4])
    far[:3, 3] += 1.0e4
    rep = scene_ctx.points_resident(far, QS)
    assert rep.points == 6000 and (rep.matched, rep.counted, rep.negative, rep.not_finite) == (0, 0, 0, 0)
    assert np.all(np.isposinf(rep.d2)) and np.all(np.isposinf(rep.sq_error)) and not rep.weight.any() and not rep.status.any()
    assert len(rep.quantiles) == len(QS) and np.isnan(rep.quantiles).all()


# ---- 6 -------------------------------------------------------------------------------------------------------------
def test_flags_of_a_nan_and_of_an_indefinite_covariance(gpu_ctx, scene, references, oracle):
    vmap, om, pts, covs, T_true, _ = scene
    n = 300
    ref = references["T_true"].prefix(n)
    a, b = int(ref.index[3]), int(ref.index[40])              # two matched points
    lam = float(np.linalg.eigvalsh(vmap.covs.reshape(-1, 3, 3)).max())
    edited = covs[:n].copy()
    edited[a] = np.nan
    edited[b] = (-4.0 * max(1.0, lam) * np.eye(3)).reshape(9)      # beyond every voxel covariance: S is negative definite
    ref_edit = pr.reference_at(oracle, om, pts[:n], edited, T_true)
    assert np.array_equal(ref_edit.index, ref.index)
    raw_a, raw_b = (float(ref_edit.raw[ref_edit.index == i][0]) for i in (a, b))
    assert np.isnan(raw_a) and raw_b < 0.0
    load_map(gpu_ctx, vmap)
    gpu_ctx.set_robust("none", 1.0, 0.04)
    gpu_ctx.scan_upload(pts[:n], covs[:n])
    plain = gpu_ctx.points_resident(T_true, QS)
    gpu_ctx.scan_upload(pts[:n], edited)
    rep = gpu_ctx.points_resident(T_true, QS)
    assert rep.status[a] == MATCHED | NOT_FINITE and rep.status[b] == MATCHED | NEGATIVE
    assert not np.isfinite(rep.d2[a]) and rep.weight[a] == 0.0            # a NaN residual fails the gate
    assert rep.d2[b] < 0.0 and rep.weight[b] == 1.0 and abs(rep.d2[b] - raw_b) <= 1e-9 * abs(raw_b)
    assert (rep.matched, rep.negative, rep.not_finite) == (plain.matched, 1, 1)
    assert rep.counted == int(np.count_nonzero(rep.weight > 0.0))
    others = np.ones(n, dtype=bool)
    others[[a, b]] = False
    for x, y in ((rep.d2, plain.d2), (rep.sq_error, plain.sq_error), (rep.weight, plain.weight), (rep.status, plain.status)):
        assert same_bits(x[others], y[others])
    assert rep.sq_error[a] == plain.sq_error[a] and rep.sq_error[b] == plain.sq_error[b]     # e does not read the covariance
    # the quantiles: the NaN point is not ranked, the negative one is ranked as 0
    ranked = (rep.status & MATCHED != 0) & (rep.status & NOT_FINITE == 0)
    assert not ranked[a] and ranked[b] and ranked.sum() == plain.matched - 1
    own = np.sort(np.maximum(rep.d2[ranked], 0.0))
    assert own[0] == 0.0 and same_bits(rep.quantiles, pr.order_statistics(own, QS)) and rep.quantiles[0] == 0.0
    assert not np.signbit(rep.quantiles[0]) and np.isfinite(rep.quantiles).all()


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_read_only(scene, gpu_ctx):
    """Around a call the scan generation and the fallback counter stand still; an align, a batch of four and an evaluation
    return the same bits with calls in between as without; one host synchronisation per call."""
    from eskf_lio_amd import capi
    vmap, _, pts, covs, T_true, guess = scene
    guesses = jitter_guesses(4)

    def run(ctx, between):
        out = []
        between(ctx)
        out.append(ctx.align_resident(guess, rr.MAX_IT, rr.TSQ, rr.COS))
        between(ctx)
        out.extend(ctx.align_resident_batch(guesses, rr.MAX_IT, rr.TSQ, rr.COS))
        between(ctx)
        out.append(ctx.align_resident(guess, rr.MAX_IT, rr.TSQ, rr.COS, flags=capi.FLAG_NO_PERSISTENT))
        between(ctx)
        ev = ctx.evaluate_resident([guess, T_true])
        between(ctx)
        return out, ev

    def report(ctx):
        before = (ctx.counter(COUNTER_SCAN_GENERATION), ctx.counter(COUNTER_FALLBACKS))
        ctx.frame_stats(reset=True)
        ctx.points_resident(guess, QS)
        assert ctx.frame_stats().host_syncs == 1
        ctx.points_resident(T_true, (), d2=False, sq_error=False, weight=False, status=False)
        assert ctx.frame_stats().host_syncs == 2
        assert (ctx.counter(COUNTER_SCAN_GENERATION), ctx.counter(COUNTER_FALLBACKS)) == before

    load_map(gpu_ctx, vmap)
    gpu_ctx.scan_upload(pts, covs)
    want, want_ev = run(gpu_ctx, lambda ctx: None)
    with capi.Context(0) as other:
        load_map(other, vmap)
        other.scan_upload(pts, covs)
        got, got_ev = run(other, report)
        assert other.counter(COUNTER_FALLBACKS) == 0
    assert len(got) == len(want) == 6
    for h, (g, w) in enumerate(zip(got, want)):
        assert_same_bits(g, w, f"call {h}")
    for g, w in zip(got_ev, want_ev):
        assert g.correspondences == w.correspondences and g.cost == w.cost and g.sq_error == w.sq_error
        assert same_bits(g.normal_eq, w.normal_eq)


# ---- 8 -------------------------------------------------------------------------------------------------------------
def test_edges(scene):
    """The header's refusals with a real context, in their order, and that a refusal writes nothing (rule 10:
    summary.points only); a pending preparation is settled; counts alone."""
    from eskf_lio_amd import capi, synth
    vmap, _, pts, covs, T_true, _ = scene
    lib = capi.load_library()
    n = pts.shape[0]
    pose = capi.pose_to_abi(T_true)
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    d2, sq, w = (np.full(n, -7.0) for _ in range(3))
    status = np.full(n, 0xA5, dtype=np.uint8)
    summary = capi.PointSummary()

    def call(ctx, pose=pose, capacity=n, arrays=True, nq=0, q=None, with_summary=True):
        C.memset(C.byref(summary), 0xA5, C.sizeof(summary))
        for x in (d2, sq, w):
            x[:] = -7.0
        status[:] = 0xA5
        qa = np.ascontiguousarray(q, dtype=np.float64) if q is not None else None
        give = (lambda x, t: x.ctypes.data_as(t)) if arrays else (lambda x, t: None)
        return lib.vgicp_points_resident(ctx._h if ctx is not None else None,
                                         pose.ctypes.data_as(dp) if pose is not None else None, capacity, give(d2, dp),
                                         give(sq, dp), give(w, dp), give(status, u8p), nq,
                                         qa.ctypes.data_as(dp) if qa is not None else None,
                                         C.byref(summary) if with_summary else None, None)

    def untouched():
        return (np.all(d2 == -7.0) and np.all(sq == -7.0) and np.all(w == -7.0) and np.all(status == 0xA5) and
                bytes(summary) == b"\xa5" * C.sizeof(summary))

    bad_pose = pose.copy()
    bad_pose[13] = np.inf
    assert call(None) == capi.ERR_BAD_ARGUMENT and untouched()                                         # 1
    with capi.Context(0) as ctx:
        # no map yet: rules 3-7 come before rule 9
        for kwargs, text in ((dict(pose=None), "NULL pose"), (dict(pose=bad_pose), "not finite"),                # 3, 4
                             (dict(nq=17, q=[0.5] * 17), "n_quantiles"), (dict(nq=1), "need q"),          # 5, 6
                             (dict(nq=1, q=[0.5], with_summary=False), "need q"),
                             (dict(nq=2, q=[0.5, 1.5]), "[0, 1]"), (dict(nq=1, q=[np.nan]), "[0, 1]"),    # 7
                             (dict(nq=1, q=[-0.1]), "[0, 1]"),
                             (dict(pose=None, nq=17), "NULL pose"), (dict(pose=bad_pose, nq=1), "not finite")):
            assert call(ctx, **kwargs) == capi.ERR_BAD_ARGUMENT and text in ctx.last_error(), (kwargs, ctx.last_error())
            assert untouched()
        assert call(ctx) == capi.ERR_NOT_READY and "map" in ctx.last_error() and untouched()            # 9
        load_map(ctx, vmap)
        assert call(ctx) == capi.ERR_NOT_READY and "scan" in ctx.last_error() and untouched()
        ctx.scan_upload(pts, covs)
        assert call(ctx, capacity=n - 1) == capi.ERR_BAD_ARGUMENT and "capacity" in ctx.last_error()     # 10
        assert summary.points == n and np.all(d2 == -7.0) and np.all(status == 0xA5)
        assert bytes(summary)[8:] == b"\xa5" * (C.sizeof(summary) - 8)
        assert call(ctx, capacity=0, arrays=False, with_summary=False) == capi.OK                        # nothing asked at all
        # counts alone
        assert call(ctx, capacity=0, arrays=False) == capi.OK and np.all(d2 == -7.0)
        counts = (summary.points, summary.matched, summary.counted, summary.negative, summary.not_finite)
        assert counts == (n, 5856, 5856, 0, 0)
        assert bytes(summary)[40:] == b"\xa5" * 128                                                   # no quantile was asked
        assert call(ctx, nq=2, q=[0.5, 1.0]) == capi.OK and np.all(np.isfinite(d2[status == 1]))
        assert (summary.points, summary.matched) == (n, 5856) and summary.quantile[0] <= summary.quantile[1]
        assert bytes(summary)[56:] == b"\xa5" * 112                                                   # beyond n_quantiles: not written
        # a pending preparation is settled: the report is of the prepared scan
        raw = synth.make_lidar_scan(3_000, seed=3)
        ctx.scan_prepare_async(raw, None, None, None, 0.3, 30)
        assert call(ctx, capacity=n) == capi.OK
        kept = ctx.scan_info()[0]
        assert 0 < kept < 3_000 and summary.points == kept
    with capi.Context([0, 0]) as multi:                                                                  # 8
        load_map(multi, vmap)
        multi.scan_upload(pts, covs)
        for arrays in (True, False):
            assert call(multi, arrays=arrays) == capi.ERR_BAD_ARGUMENT and untouched()
            assert "multi-device contexts" in multi.last_error() and "shard" in multi.last_error()
        assert call(multi, pose=None) == capi.ERR_BAD_ARGUMENT and "NULL pose" in multi.last_error()     # 3 before 8


# ---- 9 -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_shim_point_report_is_the_c_abis(scene):
    """ICP::pointReport through libvgicp_host.so.  On the cloud CloudPreprocessor::process left resident it reads the
    resident scan (no upload) and returns, bit for bit, what the C ABI returns for the same cloud on a context that holds
    the same voxels; on arrays it uploads once.  The weights are those of the ICP's own robust settings."""
    from eskf_lio_amd import capi, host, synth
    st = synth.make_imu_states(48, seed=9)
    n = 30_000
    t = synth.make_point_times(n, st[1, 0] + 1e-4, st[-3, 0] + 1e-3, seed=9)
    ext = synth.se3_to_SE3([0.01, -0.02, 0.03, 0.002, -0.001, 0.003])
    raws = [synth.make_lidar_scan(n, seed=60 + f) for f in range(2)]
    no_gate = dict(translation_sq_threshold=-1.0, cosine_threshold=2.0, remove_distant_points=False,
                   distance_threshold=1e9, removing_period=1e9, device_resident=True)
    pose = synth.se3_to_SE3([0.02, -0.01, 0.0, 0.0, 0.0, 0.004])
    pre = host.CloudPreprocessor(0.3, ext, "eager")
    icp = host.ICP(12, 1e-6, 0.9999, robust_kernel="cauchy", robust_scale=0.15, gate=0.06)
    lmap = host.LocalMap(0.3, 20, no_gate)
    first = host.Frame(raws[0], t, st)
    first.run(pre, icp, lmap, np.eye(4), first_frame=True)
    first.end()
    uploaded = lmap.counter(2)                                           # VGICP_COUNTER_UPLOAD_BYTES
    fr = host.Frame(raws[1], t, st)
    rep, used_resident = fr.pointReport(pre, icp, lmap, pose, QS)
    fr.end()
    assert used_resident and lmap.counter(2) == uploaded
    counts_only = host.Frame(raws[1], t, st)
    rep0, used0 = counts_only.pointReport(pre, icp, lmap, pose, QS, perPoint=False)
    counts_only.end()
    assert used0 and rep0.d2 is None and same_bits(rep0.quantiles, rep.quantiles) and rep0.counted == rep.counted
    gp, gc = host.CloudPreprocessor(0.3, ext, "eager").process(st, raws[1], t)
    kept = gp.shape[0]
    assert rep.points == kept == len(rep.d2) and 0 < rep.counted <= rep.matched <= kept
    arrays = icp.pointReport(gp, gc, lmap, pose, QS)
    assert not icp.used_resident and same_report(arrays, rep) and same_bits(arrays.quantiles, rep.quantiles)
    keys, means, vcovs, _ = lmap.export()
    with capi.Context(0) as ctx:
        ctx.map_reset(0.3, keys.shape[0])
        ctx.map_upsert(keys, means, vcovs)
        ctx.scan_upload(gp, gc)
        ctx.set_robust("cauchy", 0.15, 0.06)
        want = ctx.points_resident(pose, QS)
    assert same_report(rep, want) and same_bits(rep.quantiles, want.quantiles)
    assert (rep.points, rep.matched, rep.counted, rep.negative, rep.not_finite) == \
        (want.points, want.matched, want.counted, want.negative, want.not_finite)


def test_shim_scale_from_a_quantile_halves_the_error(scene, references):
    """robustScaleFromQuantile of pointReport's quantile at the guess, put into setRobust("huber", ...): the align's
    translation error against T_true is at most half the plain align's, the criterion of tests/test_robust.py.  The
    quantile is the MEDIAN: with the 0.9 quantile (0.066, c = 0.257) the reference IRLS itself does not meet the
    criterion on this scene (10.8 mm against 16.1 mm plain), with the median (0.0079, c = 0.089) it does (5.1 mm) —
    tests/test_points_cpu.py::test_reference_scale_from_a_quantile_meets_the_robust_criterion asserts both."""
    from eskf_lio_amd import capi, host
    vmap, _, pts, covs, T_true, guess = scene
    lmap = host.LocalMap(vmap.voxel_size, 1)                    # one point per voxel: the voxel IS the mean + covariance
    lmap.updateLocalMap(vmap.means, vmap.covs, np.eye(4))
    icp = host.ICP(rr.MAX_IT, rr.TSQ, rr.COS)
    plain = icp.align(pts, covs, lmap, guess)
    rep = icp.pointReport(pts, covs, lmap, guess, [0.5, 0.9], perPoint=False)
    assert rep.d2 is None and rep.matched == 5905 == rep.counted
    ref_q = pr.order_statistics(references["guess"].ranked, [0.5, 0.9])
    assert np.max(np.abs(rep.quantiles - ref_q) / ref_q) <= term_bound(references["guess"].kappa)
    c = host.ICP.robustScaleFromQuantile(rep.quantiles[0])
    assert c == math.sqrt(rep.quantiles[0]) and "%.3f" % c == "0.089"
    assert host.ICP.robustScaleFromQuantile(rep.quantiles[1], 0.5) == 0.5 * math.sqrt(rep.quantiles[1])
    for bad in (float("nan"), 0.0, -1.0):
        with pytest.raises(ValueError):
            host.ICP.robustScaleFromQuantile(bad)
    kind, c_used, _ = icp.setRobust(capi.ROBUST_HUBER, c, 0.0)
    assert kind == capi.ROBUST_HUBER and abs(c_used - c) <= 0.5e-6
    robust = icp.align(pts, covs, lmap, guess)
    err, err_plain = rr.translation_error(robust, T_true), rr.translation_error(plain, T_true)
    print(f"Huber at the median's scale {c_used}: {1e3 * err:.3f} mm against {1e3 * err_plain:.3f} mm plain")
    assert err <= 0.5 * err_plain
    # the weights of a report are the ICP's own settings now
    weighted = icp.pointReport(pts, covs, lmap, guess)
    hit = weighted.status & MATCHED != 0
    assert weighted.counted == 5905 and np.all(weighted.weight[hit] <= 1.0) and (weighted.weight[hit] < 1.0).sum() > 2000
    want_w = rr.weights(weighted.d2[hit], rr.HUBER, c_used, 0.0)[0]
    assert np.max(np.abs(weighted.weight[hit] - want_w)) <= 16 * U


@pytest.mark.timeout(600)
def test_replay_sets_the_scale_from_the_quantile_in_every_frame():
    """Six synthetic frames with registration.robust_scale_quantile = 0.9 (tools/replay.py --robust-scale-quantile 0.9) on
    the resident chain: before each frame's align the backend sets exactly the scale recomputed here from a
    points_resident call at that frame's predicted pose; kernel and gate stay as configured.  Without the key, no report is
    made and the scale is never touched."""
    from eskf_lio_amd import replay, synth
    from replay_backends import stream_events
    from test_replay import _clone
    events, _ = synth.make_sensor_stream(frames=6, points_per_frame=6_000)
    events = stream_events(replay, events)

    class Watching(replay.DeviceBackend):
        def __init__(self, cfg):
            super().__init__(cfg, 0)
            self.expected, self.reports = [], 0

        def align(self, points, covs, guess):
            if self.scale_quantile is not None:
                mine = self.ctx.points_resident(guess, [0.9], d2=False, sq_error=False, weight=False, status=False)
                self.expected.append(min(max(math.sqrt(mine.quantiles[0]), 1e-6), (2 ** 31 - 1) / 1e6))
            before = len(self.scales)
            pose = super().align(points, covs, guess)
            if self.scale_quantile is not None:
                assert len(self.scales) == before + 1
                d2q, c = self.scales[-1]
                assert c == round(self.expected[-1] * 1e6) / 1e6 and d2q == mine.quantiles[0]
                # what the context holds now, by its effect: Huber at that scale, the gate as configured
                held = self.ctx.points_resident(guess, sq_error=False)
                hit = held.status & MATCHED != 0
                want = rr.weights(held.d2[hit], rr.HUBER, c, 0.05)[0]
                assert np.max(np.abs(held.weight[hit] - want)) <= 16 * U and (want == 0.0).any() and (want == 1.0).any()
            return pose

    cfg = dict(replay.DEFAULT_CONFIG, registration=dict(replay.DEFAULT_CONFIG["registration"], robust_kernel="huber",
                                                        robust_scale=0.1, gate=0.05, robust_scale_quantile=0.9))
    backend = Watching(cfg)
    traj = replay.Odometry(cfg, backend).run([(a, _clone(m)) for a, m in events])
    assert len(traj) == 6 and len(backend.scales) == len(backend.expected) == 5      # the first frame only builds the map
    assert backend.iterations and len(backend.iterations) == 5
    assert len({c for _, c in backend.scales}) > 1 and all(1e-3 < c < 10.0 for _, c in backend.scales)
    backend.ctx.close()
    off = dict(replay.DEFAULT_CONFIG, registration=dict(replay.DEFAULT_CONFIG["registration"], robust_kernel="huber",
                                                        robust_scale=0.1, gate=0.05))
    plain = Watching(off)
    replay.Odometry(off, plain).run([(a, _clone(m)) for a, m in events])
    assert plain.scales == [] and plain.expected == []
    plain.ctx.close()
