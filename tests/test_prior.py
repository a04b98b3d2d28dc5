"""The pose prior (include/vgicp_hip_prior.h) on the device: a Gaussian prior on the pose in every round of vgicp_align,
vgicp_align_resident and vgicp_align_resident_batch.

The reference is tests/prior_reference.py's Gauss-Newton (the oracle's correspondences, per-term blocks, exponential,
compose and convergence test; the chart restated in numpy; numpy.linalg.solve), which tests/test_prior_cpu.py holds
against the library's host chart.  Scenes: robust_reference.make_scene (6 000 points, 20 000 voxels) and, for the
several-points-per-thread body, tests/test_robust.py's big_inputs / sizes_for.  Everything that compares two device paths
is bit for bit."""
import numpy as np
import pytest

import prior_reference as pr
import robust_reference as rr
from conftest import NORMAL_EQ_RTOL, TIGHT_POSE_TOL, pose_error
from test_align_batch import assert_same_bits, jitter_guesses, load_map
from test_robust import align3, sizes_for

pytestmark = pytest.mark.gpu

COUNTER_LAUNCHES, COUNTER_FALLBACKS = 0, 1
ARGS = (rr.MAX_IT, rr.TSQ, rr.COS)


def offset_pose(T, metres, degrees, seed):
    """se3ToSE3 of a step of that length and that angle (random directions), applied on the left of T."""
    from eskf_lio_amd import synth
    rng = np.random.default_rng(seed)
    v, w = rng.normal(size=3), rng.normal(size=3)
    xi = np.r_[metres * v / np.linalg.norm(v), np.radians(degrees) * w / np.linalg.norm(w)]
    return synth.se3_to_SE3(xi) @ T


def dense_spd(seed=3):
    B = np.random.default_rng(seed).normal(size=(6, 6))
    return 40.0 * (B @ B.T) + 5.0 * np.eye(6)


# the priors of the parity test: name -> information; all anchored 3 cm / 0.5 degrees off the guess
PRIORS = {
    "10 I": 10.0 * np.eye(6),
    "translation only": np.diag([1e4, 1e4, 1e4, 0.0, 0.0, 0.0]),
    "dense": dense_spd(),
}
CAUCHY = (rr.CAUCHY, 0.15, 0.0)


@pytest.fixture(scope="module")
def scene(oracle):
    vmap, pts, covs, T_true, guess = rr.make_scene()
    om = oracle.OracleMap(vmap.voxel_size, 1)
    om.insert(vmap.means, vmap.covs)
    return vmap, om, pts, covs, T_true, guess, offset_pose(guess, 0.03, 0.5, seed=21)


@pytest.fixture(scope="module")
def references(scene, oracle):
    """The reference align of every prior of the parity test, and of the dense one with Cauchy on top, computed once."""
    _, om, pts, covs, _, guess, T0 = scene
    out = {name: pr.prior_align(oracle, om, pts, covs, guess, T0, L) for name, L in PRIORS.items()}
    out["dense+cauchy"] = pr.prior_align(oracle, om, pts, covs, guess, T0, PRIORS["dense"], *CAUCHY)
    return out


@pytest.fixture()
def scene_ctx(gpu_ctx, scene):
    vmap, _, pts, covs = scene[:4]
    load_map(gpu_ctx, vmap)
    gpu_ctx.scan_upload(pts, covs)
    return gpu_ctx


@pytest.fixture(scope="module")
def big_inputs():
    from eskf_lio_amd import synth
    vmap = synth.make_map(120_000)
    pts, covs, _ = synth.make_structured_scan(256 * 448 + 1, vmap)
    return vmap, pts, covs, synth.default_guess()


def chart_norm(T0, T):
    return float(np.linalg.norm(pr.chart(T0, T)[0]))


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["persistent", "loop"])
@pytest.mark.parametrize("name", list(PRIORS) + ["dense+cauchy"])
def test_parity_with_the_reference(scene_ctx, scene, references, name, path):
    """Rounds, verdict and every round's count equal the reference's; every normal_eq row (the DATA sums) within
    NORMAL_EQ_RTOL, scaled as tests/test_robust.py scales it; the pose within TIGHT_POSE_TOL.

    Observed on an MI355X (the persistent launch and the loop alike): 3 / 4 / 3 / 9 rounds (10 I, translation only, dense,
    dense + Cauchy), normal_eq within 1.2e-11 of its scale at worst (10 I), pose within 3.5e-16 m / 8.1e-18 rad."""
    from eskf_lio_amd import capi
    _, _, _, _, _, guess, T0 = scene
    ref = references[name]
    L = PRIORS["dense" if name == "dense+cauchy" else name]
    if name == "dense+cauchy":
        scene_ctx.set_robust(*CAUCHY)
    scene_ctx.set_pose_prior(T0, L)
    flags = capi.FLAG_NO_PERSISTENT if path == "loop" else 0
    got = scene_ctx.align_resident(guess, *ARGS, flags=flags)
    assert (got.launches == 1) == (path == "persistent")
    assert got.iterations == ref.iterations and got.converged == ref.converged, (got.iterations, ref.iterations)
    assert np.array_equal(got.corr_count, ref.corr_count), (got.corr_count, ref.corr_count)
    worst = 0.0
    for it in range(ref.iterations):
        g, r = got.normal_eq[it], ref.normal_eq[it]
        scale_J, scale_r = np.abs(r[:21]).max(), max(np.abs(r[21:]).max(), 1.0)
        d_J, d_r = np.abs(g[:21] - r[:21]).max() / scale_J, np.abs(g[21:] - r[21:]).max() / scale_r
        worst = max(worst, d_J, d_r)
        assert d_J <= NORMAL_EQ_RTOL and d_r <= NORMAL_EQ_RTOL, (it, d_J, d_r)
    dt, dr = pose_error(got.pose, ref.pose)
    print(f"{name} / {path}: rounds {got.iterations}, worst normal_eq difference {worst:.3e} of its scale, pose {dt:.3e} m "
          f"{dr:.3e} rad, |d| {chart_norm(T0, got.pose):.4e}")
    assert dt <= TIGHT_POSE_TOL and dr <= TIGHT_POSE_TOL
    assert scene_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["never set", "set then cleared", "all-zero information"])
def test_no_prior_is_the_plain_paths_bits(scene, how):
    """vgicp_align, vgicp_align_resident (both paths) and vgicp_align_resident_batch of a context whose prior is off
    return the bits of a context that never heard of the feature, and VGICP_COUNTER_PERSISTENT_LAUNCHES moves as it does
    there (a fused launch for vgicp_align, a team launch for the batch)."""
    from eskf_lio_amd import capi
    vmap, _, pts, covs, _, guess, T0 = scene
    guesses = jitter_guesses(3)

    def run(ctx):
        load_map(ctx, vmap)
        out, counts = [], []
        for call in (lambda: ctx.align(pts, covs, guess, *ARGS),
                     lambda: ctx.align_resident(guess, *ARGS),
                     lambda: ctx.align_resident(guess, *ARGS, flags=capi.FLAG_NO_PERSISTENT)):
            before = ctx.counter(COUNTER_LAUNCHES)
            out.append(call())
            counts.append(ctx.counter(COUNTER_LAUNCHES) - before)
        before = ctx.counter(COUNTER_LAUNCHES)
        batch = ctx.align_resident_batch(guesses, *ARGS)
        counts.append(ctx.counter(COUNTER_LAUNCHES) - before)
        return out, batch, counts, ctx.align_batch_width()

    with capi.Context(0) as plain_ctx:
        want, want_batch, want_counts, want_width = run(plain_ctx)
    with capi.Context(0) as ctx:
        if how == "set then cleared":
            ctx.set_pose_prior(T0, PRIORS["dense"])
            ctx.clear_pose_prior()
        elif how == "all-zero information":
            ctx.set_pose_prior(T0, PRIORS["dense"])
            ctx.set_pose_prior(T0, np.zeros((6, 6)))
        got, got_batch, got_counts, got_width = run(ctx)
        assert ctx.counter(COUNTER_FALLBACKS) == 0
    for what, a, b in zip(("host buffers", "persistent", "loop"), got, want):
        assert_same_bits(a, b, f"{how}: {what}")
        assert a.launches == b.launches
    assert got_batch.hypotheses_per_launch == want_batch.hypotheses_per_launch > 1 and got_batch.launches == want_batch.launches
    for h in range(3):
        assert_same_bits(got_batch[h], want_batch[h], f"{how}: hypothesis {h}")
    assert got_counts == want_counts and got_counts[0] == 1 and got_counts[2] == 0, (got_counts, want_counts)
    assert got_width == want_width > 1


# ---- 3 -------------------------------------------------------------------------------------------------------------
def test_round_zero_does_not_see_the_prior(gpu_ctx, scene, big_inputs):
    """corr_count[0] and normal_eq[0] are the DATA sums at the guess: bit for bit the plain align's, on both scenes and
    both paths, while the later rounds differ."""
    from eskf_lio_amd import capi
    vmap, _, pts, covs, _, guess, T0 = scene
    bvmap, bpts, bcovs, bguess = big_inputs
    for (m, p, c, g) in ((vmap, pts, covs, guess), (bvmap, bpts, bcovs, bguess)):
        load_map(gpu_ctx, m)
        n = len(p) if m is vmap else sizes_for(gpu_ctx)[1][-1]
        gpu_ctx.scan_upload(p[:n], c[:n])
        prior_pose = T0 if m is vmap else offset_pose(g, 0.03, 0.5, seed=22)
        for flags in (0, capi.FLAG_NO_PERSISTENT):
            gpu_ctx.clear_pose_prior()
            plain = gpu_ctx.align_resident(g, 6, 1e-12, 2.0, flags=flags)
            gpu_ctx.set_pose_prior(prior_pose, PRIORS["dense"])
            got = gpu_ctx.align_resident(g, 6, 1e-12, 2.0, flags=flags)
            assert got.iterations == plain.iterations == 6 and got.corr_count[0] == plain.corr_count[0] > 0
            assert np.array_equal(got.normal_eq[0], plain.normal_eq[0]), (n, flags)
            assert not np.array_equal(got.normal_eq[1], plain.normal_eq[1]) and not np.array_equal(got.pose, plain.pose)
    assert gpu_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- 4 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["persistent", "loop"])
def test_known_answer_without_data(scene_ctx, scene, path):
    """A scan 1 km from the map matches nothing in any round; with L = I the align walks to the prior pose: the rotation
    is exact after one step (Jr^-1(phi) phi = phi), the translation after two, the third step is zero and converges."""
    from eskf_lio_amd import capi
    _, _, pts, covs, _, guess, _ = scene
    T0 = offset_pose(guess, 0.4, 20.0, seed=23)
    scene_ctx.scan_upload(pts + 1000.0, covs)
    scene_ctx.set_pose_prior(T0, np.eye(6))
    got = scene_ctx.align_resident(guess, *ARGS, flags=capi.FLAG_NO_PERSISTENT if path == "loop" else 0,
                                   allow_degenerate=True)
    dt, dr = pose_error(got.pose, T0)
    print(f"{path}: rounds {got.iterations}, {dt:.3e} m {dr:.3e} rad from the prior pose")
    assert got.status == 0 and got.converged and got.iterations <= 3
    assert not got.corr_count.any() and not got.normal_eq.any()
    assert dt <= 1e-12 and dr <= 1e-12 and np.abs(got.pose - T0).max() <= 1e-12


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_strength(scene_ctx, scene):
    """L = lambda I: |d(T_lambda)| does not grow with lambda; a vanishing prior gives the plain pose (within 1e-6), an
    overwhelming one (1e12) the prior pose (within 1e-9).  Guess and prior pose differ, so mixing the two up fails.

    Where the prior pose has to sit for the last bound to be attainable at all: the minimiser obeys
    (A + lambda I) d* = -b(T0) to first order, b(T0) the data's gradient at the prior pose, so at lambda = 1e12 it stays
    |b(T0)| / 1e12 away from the prior pose, and b(T0) ~ A delta for a prior pose delta away from the data's own optimum.
    On this scene A's eigenvalues are 0.95e5 - 1.03e5 (translation) and 1.77e6 - 1.87e6 (rotation) — the oracle's
    accumulate at the oracle's plain pose — so 1e-9 needs delta below 1e-2 m and 5e-4 rad.  The prior pose is the ORACLE's
    plain pose moved by 1 mm and 0.002 degrees (3.5e-5 rad): 1e-10 m and 7e-11 rad expected, a tenth of the bound.  (With
    the prior 3 cm / 0.5 degrees off the guess, 4 cm from that optimum, the device returns 2.5e-9 m: the same formula.)
    The differences between lambda = 1e-6 and 1 are then 1e-8 of |d|, so the rounds run until a step is below 1e-9 m and
    the cosine of its angle rounds to 1.

    Observed on an MI355X: |d| = 9.985418e-04, 9.985314e-04, 9.882367e-04, 1.24e-10 for lambda = 1e-6, 1, 1e3, 1e12; at
    1e-6 the plain pose within 1.1e-14 m / 1.9e-16 rad; at 1e12 the prior pose within 9.4e-11 m / 8.1e-11 rad."""
    _, om, pts, covs, _, guess, _ = scene
    args = (rr.MAX_IT, 1e-18, 1.0)
    optimum = om.align(pts, covs, guess, *ARGS).pose
    T0 = offset_pose(optimum, 1e-3, 0.002, seed=24)
    plain = scene_ctx.align_resident(guess, *args)
    assert plain.converged and max(pose_error(plain.pose, optimum)) <= 1e-6
    assert chart_norm(T0, guess) > 2e-3 and chart_norm(T0, plain.pose) > 9e-4      # three apart: guess, prior pose, optimum
    norms, poses = [], {}
    for lam in (1e-6, 1.0, 1e3, 1e12):
        scene_ctx.set_pose_prior(T0, lam * np.eye(6))
        got = scene_ctx.align_resident(guess, *args)
        assert got.converged, lam
        norms.append(chart_norm(T0, got.pose))
        poses[lam] = got.pose
    print("lambda 1e-6, 1, 1e3, 1e12: |d| = " + ", ".join(f"{v:.6e}" for v in norms) +
          f"; plain {chart_norm(T0, plain.pose):.6e}; at 1e-6 from the plain pose " +
          "%.3e m %.3e rad; at 1e12 from the prior pose %.3e m %.3e rad" % (pose_error(poses[1e-6], plain.pose) +
                                                                           pose_error(poses[1e12], T0)))
    assert all(b <= a for a, b in zip(norms, norms[1:])), norms
    assert norms[2] < 0.999 * norms[0] and norms[3] < 1e-6 * norms[0]
    dt, dr = pose_error(poses[1e-6], plain.pose)
    assert dt <= 1e-6 and dr <= 1e-6
    dt, dr = pose_error(poses[1e12], T0)
    assert dt <= 1e-9 and dr <= 1e-9


# ---- 6 -------------------------------------------------------------------------------------------------------------
def test_prior_paths_agree_with_each_other(gpu_ctx, big_inputs):
    """With a prior set: persistent against loop (bit for bit while both partition the points alike, else within the
    tolerances tests/test_gpu_parity.py uses for the same pair of plain paths), host buffers against upload + resident, a
    second run against the first; one launch, no give-up.  The last size runs the several-points-per-thread body."""
    vmap, pts, covs, guess = big_inputs
    load_map(gpu_ctx, vmap)
    gpu_ctx.set_pose_prior(offset_pose(guess, 0.03, 0.5, seed=22), PRIORS["dense"])
    grid, sizes = sizes_for(gpu_ctx)
    for n in sizes:
        one, loop, host = align3(gpu_ctx, pts[:n], covs[:n], guess)
        assert one.launches == 1 and loop.launches > 1 and one.iterations == loop.iterations == 6
        assert np.array_equal(one.corr_count, loop.corr_count), n
        if n <= grid * 448:
            assert_same_bits(one, loop, f"n {n} persistent / loop")
        else:                                                   # the loop uses more, smaller workgroups
            assert np.allclose(one.normal_eq, loop.normal_eq, rtol=1e-11, atol=1e-7), n
            assert max(pose_error(one.pose, loop.pose)) <= TIGHT_POSE_TOL
        assert_same_bits(host, one, f"n {n} host buffers / resident")
        again = gpu_ctx.align_resident(guess, 6, 1e-12, 2.0, allow_degenerate=True)
        assert_same_bits(again, one, f"n {n} second run")
    assert gpu_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_batch_under_one_prior_is_the_single_calls(scene_ctx, scene):
    """Three guesses under one prior: three single aligns, bit for bit, one hypothesis per launch; the team launch's
    width is back once the prior is cleared."""
    T0 = scene[6]
    guesses = jitter_guesses(3)
    width = scene_ctx.align_batch_width()
    assert width > 1
    scene_ctx.set_pose_prior(T0, PRIORS["dense"])
    want = [scene_ctx.align_resident(g, *ARGS, allow_degenerate=True) for g in guesses]
    got = scene_ctx.align_resident_batch(guesses, *ARGS)
    assert got.hypotheses_per_launch == 1 and got.launches == 3 and scene_ctx.align_batch_width() == 1
    for h in range(3):
        assert_same_bits(got[h], want[h], f"hypothesis {h}")
        assert want[h].launches == 1
    scene_ctx.clear_pose_prior()
    assert scene_ctx.align_batch_width() == width
    assert scene_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- 8 -------------------------------------------------------------------------------------------------------------
def test_bystanders_ignore_the_prior(scene_ctx, scene):
    """vgicp_evaluate_resident, vgicp_accumulate and vgicp_solve_step return the same bits with and without a prior."""
    _, _, pts, covs, _, guess, T0 = scene

    def bystanders():
        scored = scene_ctx.evaluate_resident([guess, T0])
        acc = scene_ctx.accumulate(pts, covs, guess)
        scene_ctx.scan_upload(pts, covs)
        return scored, acc, scene_ctx.solve_step(acc[0], acc[1], rr.COS, rr.TSQ)

    off = bystanders()
    scene_ctx.set_pose_prior(T0, PRIORS["dense"])
    on = bystanders()
    for a, b in zip(on[0], off[0]):
        assert a.correspondences == b.correspondences and a.cost == b.cost and a.sq_error == b.sq_error
        assert np.array_equal(a.normal_eq, b.normal_eq)
    assert on[1][2] == off[1][2] > 0 and np.array_equal(on[1][0], off[1][0]) and np.array_equal(on[1][1], off[1][1])
    assert np.array_equal(on[2][0], off[2][0]) and np.array_equal(on[2][1], off[2][1]) and on[2][2:] == off[2][2:]
    # and the prior is in force all the same
    with_prior = scene_ctx.align_resident(guess, *ARGS)
    scene_ctx.clear_pose_prior()
    assert not np.array_equal(with_prior.pose, scene_ctx.align_resident(guess, *ARGS).pose)


# ---- 9 -------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(scene_ctx, scene):
    """Every item of the header's refusal list is VGICP_ERR_BAD_ARGUMENT with a text and leaves the prior that was set
    before in force (the next align returns its bits); a communicator of one rank refuses the align."""
    from eskf_lio_amd import capi
    _, _, _, _, _, guess, T0 = scene
    L = PRIORS["dense"]
    scene_ctx.set_pose_prior(T0, L)
    want = scene_ctx.align_resident(guess, *ARGS)

    def with_entry(M, r, c, v):
        out = np.array(M, dtype=np.float64)
        out[r, c] = v
        return out

    skewed = T0.copy()
    skewed[:3, 0] *= 1.0 + 1e-8                                  # a column of length 1 + 1e-8
    sheared = T0.copy()
    sheared[:3, 1] += 1e-8 * sheared[:3, 0]                      # two columns 1e-8 from orthogonal
    indefinite = L - 1.001 * np.linalg.eigvalsh(L).min() * np.eye(6)
    hollow = np.zeros((6, 6))
    hollow[0, 1] = hollow[1, 0] = 1.0                            # zero diagonal, not positive semi-definite
    bad = {
        "information nan": (T0, with_entry(L, 2, 2, np.nan)),
        "information inf": (T0, with_entry(L, 4, 1, np.inf)),
        "pose nan": (with_entry(T0, 1, 3, np.nan), L),
        "asymmetric": (T0, with_entry(L, 5, 0, L[5, 0] + 1e-11 * np.abs(L).max())),
        "indefinite": (T0, indefinite),
        "hollow": (T0, hollow),
        "negative diagonal": (T0, np.diag([1.0, 1.0, 1.0, 1.0, 1.0, -1e-6])),
        "column length": (skewed, L),
        "columns not orthogonal": (sheared, L),
        "last row": (with_entry(T0, 3, 3, 1.0 + 1e-15), L),
        "last row, off diagonal": (with_entry(T0, 3, 0, 1e-300), L),
    }
    for what, (pose, info) in bad.items():
        with pytest.raises(capi.VgicpError) as e:
            scene_ctx.set_pose_prior(pose, info)
        assert e.value.code == capi.ERR_BAD_ARGUMENT and len(str(e.value)) > 30, what
        assert_same_bits(scene_ctx.align_resident(guess, *ARGS), want, f"after the refused {what}")
    # what is inside the tolerances is taken: an asymmetry of 1e-13 max|L|, a semi-definite L
    scene_ctx.set_pose_prior(T0, with_entry(L, 5, 0, L[5, 0] + 1e-13 * np.abs(L).max()))
    v = np.random.default_rng(1).normal(size=(6, 2))
    scene_ctx.set_pose_prior(T0, v @ v.T)                        # rank 2
    scene_ctx.set_pose_prior(T0, L)
    # a multi-device context refuses the call itself, with a text
    with capi.Context([0, 0]) as multi:
        with pytest.raises(capi.VgicpError) as e:
            multi.set_pose_prior(T0, L)
        assert e.value.code == capi.ERR_BAD_ARGUMENT and "single-device" in str(e.value)
        # ... but a clear is never refused and leaves vgicp_last_error's text alone
        multi.clear_pose_prior()
        assert b"single-device" in multi._lib.vgicp_last_error(multi._h)
    # a communicator of one rank: the align is refused while the prior is set, and runs again once it is cleared
    scene_ctx.comm_init(1, 0, scene_ctx.comm_unique_id())
    with pytest.raises(capi.VgicpError) as e:
        scene_ctx.align_resident(guess, *ARGS)
    assert e.value.code == capi.ERR_BAD_ARGUMENT and "vgicp_hip_prior.h" in str(e.value)
    scene_ctx.clear_pose_prior()
    assert scene_ctx.align_resident(guess, *ARGS).converged
    scene_ctx.comm_destroy()
    scene_ctx.set_pose_prior(T0, L)
    assert_same_bits(scene_ctx.align_resident(guess, *ARGS), want, "after the communicator is gone")


# ---- 10 ------------------------------------------------------------------------------------------------------------
def test_shim_align_with_prior_returns_the_c_abis_pose(scene):
    """ESKF_LIO::ICP::alignWithPrior through libvgicp_host.so: the C ABI's pose bit for bit, its posterior information
    G^-T A G^-1 + L from the C ABI's own pieces, and no prior left behind on the ICP or on the shared context."""
    from eskf_lio_amd import capi, host
    vmap, _, pts, covs, _, guess, _ = scene
    L = PRIORS["dense"]
    lmap = host.LocalMap(vmap.voxel_size, 1)                    # one point per voxel: the voxel IS the mean + covariance
    lmap.updateLocalMap(vmap.means, vmap.covs, np.eye(4))
    keys, means, vcovs, _ = lmap.export()
    with capi.Context(0) as ctx:
        ctx.map_reset(vmap.voxel_size, keys.shape[0])
        ctx.map_upsert(keys, means, vcovs)
        plain = ctx.align(pts, covs, guess, *ARGS)
        ctx.set_pose_prior(guess, L)                            # alignWithPrior anchors the prior at the guess
        want = ctx.align(pts, covs, guess, *ARGS)
        ctx.clear_pose_prior()
        posterior = capi.posterior_information(ctx.evaluate_resident([want.pose])[0].normal_eq, guess, want.pose, L)
    assert not np.array_equal(want.pose, plain.pose)
    icp = host.ICP(*ARGS)
    pose = icp.alignWithPrior(pts, covs, lmap, guess, L)
    assert np.array_equal(pose, want.pose) and icp.iterations == want.iterations and icp.converged == want.converged
    assert not icp.prior_left_behind
    got = icp.posteriorInformation()
    assert np.allclose(got, got.T, rtol=1e-12, atol=0) and np.allclose(got, posterior, rtol=1e-11, atol=0)
    assert np.array_equal(icp.align(pts, covs, lmap, guess), plain.pose)              # nothing left on the context
    assert np.array_equal(host.ICP(*ARGS).align(pts, covs, lmap, guess), plain.pose)


# ---- 11 ------------------------------------------------------------------------------------------------------------
def test_replay_with_the_iterated_update():
    """Twelve synthetic frames of 6 000 points (tests/test_replay.py's frame size) through Odometry::run's loop with
    kalman_filter.update.iterated: every align converges, the trajectory is finite, and the end-point error against the
    synthetic ground truth is at most 1.5 x the plain update's on the same stream (the reference's behaviour).

    Measured on an MI355X (profiles/r28_prior.txt): 2.337 mm with the iterated update, 2.229 mm with the plain one,
    ratio 1.048; 1 - 3 rounds per frame, every align converged."""
    from eskf_lio_amd import replay, synth
    from replay_backends import stream_events
    raw, truth = synth.make_sensor_stream(frames=12, points_per_frame=6_000)

    def run(config):
        backend = replay.DeviceBackend(config, 0)
        try:
            traj = replay.Odometry(config, backend).run(stream_events(replay, raw))
        finally:
            backend.ctx.close()
        return traj, backend

    plain_traj, _ = run(replay.DEFAULT_CONFIG)
    config = dict(replay.DEFAULT_CONFIG, kalman_filter=dict(replay.DEFAULT_CONFIG["kalman_filter"], iterated=True))
    traj, backend = run(config)
    assert len(traj) == len(plain_traj) == len(truth) == 12
    assert len(backend.converged) == 11 and all(backend.converged), backend.converged
    assert all(np.isfinite(T).all() for _, T in traj)
    err_plain = float(np.linalg.norm(plain_traj[-1][1][:3, 3] - truth[-1][1][:3, 3]))
    err = float(np.linalg.norm(traj[-1][1][:3, 3] - truth[-1][1][:3, 3]))
    print(f"end-point error after 12 frames: iterated update {1e3 * err:.3f} mm, plain update {1e3 * err_plain:.3f} mm, "
          f"ratio {err / err_plain:.3f}; rounds per frame {backend.iterations}")
    assert err <= 1.5 * err_plain
