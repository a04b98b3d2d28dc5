"""One correspondence's term on the device over its domain: accumulate_match, inverse3_cofactor, rcp_newton and
robust_weight of eskf_lio_amd/csrc/vgicp_kernels.hip, the cost / squared-error slots of evaluate_kernel and the per-point
report's point_term (match_weight and mahalanobis are the term's one definition, called by all three), against
tests/match_term_reference.py (60-digit arithmetic; the bound is derived there), which tests/test_match_term_cpu.py holds
against the oracle and shows to have teeth.

Every input is ONE resident scan point: a row of vgicp_evaluate_resident or of a one-round align is one term."""
import numpy as np
import pytest

import match_term_reference as mt
from test_align_batch import load_map

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(mt.unavailable_reason() is not None, reason=str(mt.unavailable_reason()))]

TSQ, COS = 1e-12, 2.0                 # cosine threshold 2: a round never converges, max_iteration ends the align
COUNTER_FALLBACKS = 1
KERNEL_NAMES = {mt.NONE: "gate only", mt.HUBER: "Huber", mt.CAUCHY: "Cauchy"}


@pytest.fixture(scope="module")
def swept():
    vmap, groups = mt.sweep()
    return vmap, groups, mt.references()


class SweepMap:
    def __init__(self, vmap):
        self.voxel_size = mt.VOXEL
        self.keys, self.means, self.covs = vmap.arrays()


def upload(ctx, g):
    ctx.scan_upload(g.x[None], g.C9[None])


def row_of(r):
    """Slots 0-27 of round 0 of a one-round align: the 27 sums and the count."""
    assert r.iterations == 1
    return np.r_[r.normal_eq[0], float(r.corr_count[0])]


def one_round(ctx, pose, flags=0):
    from eskf_lio_amd import capi
    r = ctx.align_resident(pose, 1, TSQ, COS, flags=flags, allow_degenerate=True)
    assert (r.launches == 1) == (flags & capi.FLAG_NO_PERSISTENT == 0)
    return row_of(r)


def evaluate_rows(ctx, poses):
    """evaluate_resident in calls of at most 64 poses: per pose (slots 0-27, the 29 values of the reference)."""
    out = []
    for at in range(0, len(poses), 64):
        for ev in ctx.evaluate_resident(poses[at:at + 64]):
            assert ev.points == 1
            out.append((np.r_[ev.normal_eq, float(ev.correspondences)], np.r_[ev.normal_eq, ev.cost, ev.sq_error]))
    return out


# ---- the plain term ----------------------------------------------------------------------------------------------------
def test_the_plain_term_over_its_domain(gpu_ctx, swept):
    """Per group one scan_upload of its point and one evaluate_resident of its poses; one match per pose, so a row is one
    term: count 1, slots 0-26, the cost and |e|^2 each within its bound (match_term_reference's docstring: B_W = 100 u
    rho / l3 on W for a symmetric S, times |p|_1 per [p]x factor and |e|_1 per e factor, plus the products' roundings),
    the anchors with ==.  The indefinite groups: every value finite, a negative cost returned negative (evaluate does not
    clamp).

    Observed on an MI355X, worst |difference| / bound per axis (J^T W J / J^T W e / cost / |e|^2): scale 0.005 / 0.004 /
    0.003 / 0.227, conditioning 0.013 / 0.008 / 0.007 / 0.206, indefinite 0.004 / 0.004 / 0.004 / 0.291, asymmetry 0.010 /
    0.004 / 0.003 / 0.227, distance 0.009 / 0.005 / 0.003 / 0.197, the anchors equal (One term over
    its domain).  The numpy restatement of tests/test_match_term_cpu.py, which does not contract, reaches 0.30."""
    vmap, groups, refs = swept
    load_map(gpu_ctx, SweepMap(vmap))
    worst, negative = {}, 0
    for g in groups:
        upload(gpu_ctx, g)
        rows = evaluate_rows(gpu_ctx, [c.pose for c in g.cases])
        for k, (c, (slots, values)) in enumerate(zip(g.cases, rows)):
            t = refs[(g.name, k)]
            what = (g.name, c.label)
            assert slots[27] == 1.0, what
            assert np.isfinite(values).all(), what
            bounds, diff = t.bounds(), t.differences(values)
            if g.exact:
                assert np.array_equal(values, t.f64), (what, values, t.f64)
            ratio = np.where(bounds > 0, diff / np.where(bounds > 0, bounds, 1.0), np.where(diff > 0, np.inf, 0.0))
            worst[g.name] = np.maximum(worst.get(g.name, 0.0), [ratio[:21].max(), ratio[21:27].max(), ratio[27], ratio[28]])
            assert (ratio <= 1.0).all(), (what, ratio)
            if t.raw < 0:
                assert values[27] < 0.0, what
                negative += 1
    for name, r in worst.items():
        print(f"{name}: worst |difference| / bound: J^T W J {r[0]:.3f}, J^T W e {r[1]:.3f}, cost {r[2]:.3f}, |e|^2 {r[3]:.3f}")
    by_axis = {}
    for g in groups:
        by_axis[g.axis] = np.maximum(by_axis.get(g.axis, 0.0), worst[g.name])
    for axis, r in by_axis.items():
        print(f"axis {axis}: J^T W J {r[0]:.3f}, J^T W e {r[1]:.3f}, cost {r[2]:.3f}, |e|^2 {r[3]:.3f}")
    assert negative >= 12 and len(worst) == len(groups)
    assert gpu_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- the per-point report's term ---------------------------------------------------------------------------------------
def test_the_per_point_report_forms_the_same_term(gpu_ctx, swept):
    """The third user of the term: for every case of every group, points_resident at the case's pose (no quantiles) reports
    the one point MATCHED with d2[0] == the cost and sq_error[0] == the squared error of evaluate_resident at that pose —
    with ==: the evaluation's row is one term added to +0.0 — and weight 1.0 at the default robust options.  Where the
    reference's raw residual is negative the report's is too, with POINT_NEGATIVE set.  465 cases, 12 of them negative,
    on an MI355X."""
    from eskf_lio_amd import capi
    vmap, groups, refs = swept
    load_map(gpu_ctx, SweepMap(vmap))
    checked, negative = 0, 0
    for g in groups:
        upload(gpu_ctx, g)
        rows = evaluate_rows(gpu_ctx, [c.pose for c in g.cases])
        for k, (c, (_, values)) in enumerate(zip(g.cases, rows)):
            what = (g.name, c.label)
            rep = gpu_ctx.points_resident(c.pose)
            assert rep.points == 1 and rep.matched == 1, what
            assert rep.status[0] & capi.POINT_MATCHED, (what, rep.status[0])
            assert rep.d2[0] == values[27], (what, rep.d2[0], values[27])
            assert rep.sq_error[0] == values[28], (what, rep.sq_error[0], values[28])
            assert rep.weight[0] == 1.0, (what, rep.weight[0])
            if refs[(g.name, k)].raw < 0:
                assert rep.d2[0] < 0.0 and rep.status[0] & capi.POINT_NEGATIVE, (what, rep.d2[0], rep.status[0])
                negative += 1
            checked += 1
    print(f"{checked} cases, {negative} with a negative raw residual: the report's term equals the evaluation's")
    assert negative >= 12 and checked == sum(len(g.cases) for g in groups)
    assert gpu_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- every path, the same bits -----------------------------------------------------------------------------------------
def test_every_path_computes_the_same_bits_at_the_edges(gpu_ctx, swept):
    """Every eighth case of the sweep and every anchor, asymmetric and indefinite case: row 0 of align_resident(pose, 1)
    on the persistent launch, the same with VGICP_FLAG_NO_PERSISTENT, vgicp_accumulate and hypothesis 0 of a two-guess
    align_resident_batch all equal evaluate's slots 0-27 (DESIGN.md's promise, so far held on synth's inputs only).
    148 cases on an MI355X."""
    from eskf_lio_amd import capi
    vmap, groups, _ = swept
    load_map(gpu_ctx, SweepMap(vmap))
    number, checked = 0, 0
    with capi.Context(0) as other:                            # vgicp_accumulate replaces the resident scan
        load_map(other, SweepMap(vmap))
        for g in groups:
            chosen = []
            for c in g.cases:
                if number % 8 == 0 or g.axis in ("anchor", "asymmetry", "indefinite"):
                    chosen.append(c)
                number += 1
            if not chosen:
                continue
            upload(gpu_ctx, g)
            rows = evaluate_rows(gpu_ctx, [c.pose for c in chosen])
            for c, (want, _) in zip(chosen, rows):
                what = (g.name, c.label)
                assert np.array_equal(one_round(gpu_ctx, c.pose), want), (what, "persistent")
                assert np.array_equal(one_round(gpu_ctx, c.pose, capi.FLAG_NO_PERSISTENT), want), (what, "loop")
                JTJ, JTr, count = other.accumulate(g.x[None], g.C9[None], c.pose)
                got = np.r_[[JTJ[r, col] for r, col in mt.SLOTS], JTr, float(count)]
                assert np.array_equal(got, want), (what, "accumulate")
                batch = gpu_ctx.align_resident_batch([c.pose, chosen[0].pose], 1, TSQ, COS)
                assert np.array_equal(row_of(batch[0]), want), (what, "batch")
                checked += 1
    print(f"{checked} cases, four paths each, equal to evaluate's row")
    assert checked >= 103 + 40                                # 4 anchor, 51 asymmetric, 48 indefinite cases and every eighth of the rest
    assert gpu_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- the weight --------------------------------------------------------------------------------------------------------
def test_the_robust_weight_over_its_domain(gpu_ctx, swept):
    """One-round robust aligns of one point, on the persistent launch and on the loop (their rows are equal), under Huber
    and Cauchy with c = 1 and 2, the gate alone at 1 and 4, and Cauchy with a gate — values the library holds exactly
    (asserted on set_robust's read-back).  Every weighted slot within w_ref x (the plain bound) + 4 u of w_ref x (the
    reference slot), the count (w_ref > 0):
      - d^2 from 1e-12 to 1e12 times c^2 (times the gate), with 20 values within 1e-12 relative of c^2 on both sides: Huber
        is continuous there, nothing is left out; tests/test_match_term_cpu.py shows every gated case decidable
      - S = I exactly: e = (1, 0, 0) against the gate 1.0 is kept, e = (1 + 2^-52, 0, 0) is rejected and every slot is +-0;
        d^2 = c^2 under Huber is the plain row's bits; every row whose weight and products are fp64 numbers is met with ==
      - e = 0 exactly: Huber's rsq(0) does not leak, the row is the plain row's bits
      - a negative raw residual (the indefinite class): d^2 is 0, the weight is 1 and the gate is passed — the plain bits.

    Observed on an MI355X, worst |difference| / bound: Huber c = 1 / 2: 0.010 / 0.003, Cauchy c = 1 / 2: 0.005 / 0.017, the
    gate alone at 1 / 4: 0.001 / 0.003, Cauchy c = 1 with gate 4: 0.005, c = 2 with gate 1: 0.008; 99 rejected rows, 22 rows
    met with == (One term over its domain)."""
    from eskf_lio_amd import capi
    vmap, _, _ = swept
    load_map(gpu_ctx, SweepMap(vmap))
    worst, rejected, exact = {}, 0, 0
    for g in mt.weight_groups():
        kernel, c, gate = g.robust
        assert gpu_ctx.set_robust(kernel, c, gate) == (kernel, c, gate)
        upload(gpu_ctx, g)
        plain = evaluate_rows(gpu_ctx, [case.pose for case in g.cases])          # evaluate stays unweighted
        setting = f"{KERNEL_NAMES[kernel]} c {c:g} gate {gate:g}"
        for case, (plain_row, _) in zip(g.cases, plain):
            what = (g.name, case.label)
            t = mt.term(case.R, case.p, g.C9, vmap.means[case.voxel], vmap.covs[case.voxel])
            ref = mt.weighted_row(t, kernel, c, gate)
            got = one_round(gpu_ctx, case.pose)
            assert np.array_equal(one_round(gpu_ctx, case.pose, capi.FLAG_NO_PERSISTENT), got), (what, "loop")
            assert got[27] == float(ref.counted), (what, got[27], ref.counted)
            ratio = ref.ratios(got[:27])
            worst[setting] = max(worst.get(setting, 0.0), float(ratio.max()))
            assert (ratio <= 1.0).all(), (what, ratio)
            if not ref.counted:
                assert not got[:27].any(), what                # +-0, every one
                rejected += 1
            if g.exact and ref.representable:
                assert np.array_equal(got[:27], [float(v) for v in ref.values]), what
                exact += 1
            if "negative" in g.name:
                assert t.raw < 0 and ref.w == 1.0 and ref.counted, what
            if (g.exact or "negative" in g.name) and ref.w == 1.0:
                assert np.array_equal(got, plain_row), (what, "the plain row's bits")
        gpu_ctx.set_robust()
    for setting, ratio in worst.items():
        print(f"{setting}: worst |difference| / bound {ratio:.3f}")
    print(f"{rejected} rejected rows, {exact} rows met with ==")
    assert len(worst) == len(mt.SETTINGS) and rejected >= 40 and exact >= 20
    assert gpu_ctx.counter(COUNTER_FALLBACKS) == 0


# ---- non-finite entries (last in the file) -----------------------------------------------------------------------------
def nan_scene(vmap, groups):
    """448 good points around the mean of the unit-scale voxel (all matched, d^2 < 0.2) and one more point in the same
    voxel, the last of the scan (so it is the second workgroup's only point), whose covariance gets one bad entry."""
    g = [g for g in groups if g.name == "scale C 1 C_voxel 1"][0]
    voxel = g.cases[0].voxel
    rng = np.random.default_rng(448)
    pts = vmap.means[voxel] + rng.uniform(-0.05, 0.05, size=(449, 3))
    covs = np.tile(g.C9, (449, 1))
    assert all(tuple(np.floor(p / mt.VOXEL).astype(int)) == vmap.keys[voxel] for p in pts)
    return pts, covs


@pytest.mark.parametrize("bits", [0x7FF8000000000000, 0xFFFFFFFFFFFFFFFF], ids=["NaN", "the unset pattern"])
def test_a_non_finite_covariance_entry(gpu_ctx, swept, bits):
    """A scan of 448 good points plus one point in an occupied voxel whose covariance has one NaN entry — the canonical
    NaN, and the all-ones pattern the persistent exchange uses for "not there yet" (publishable() rewrites it).
      - the plain align, on the loop and on the persistent launch, returns VGICP_ERR_DEGENERATE; nothing is raised, and
        the persistent fall-back counter stays where it was: the NaN crossed the exchange as a value, no poll ran out
      - with a gate set the point is rejected: row 0's count is 448, every sum is finite and the row equals the row of
        the scan without that point — what "a NaN residual is rejected" (include/vgicp_hip_robust.h) has to mean.
    Observed on an MI355X before accumulate_match selected W = 0 for a rejected correspondence (it multiplied by the
    weight 0): count 448 and all 27 sums NaN, on both paths and for both patterns."""
    from eskf_lio_amd import capi
    vmap, groups, _ = swept
    load_map(gpu_ctx, SweepMap(vmap))
    pts, covs = nan_scene(vmap, groups)
    covs = covs.copy()
    covs[448, 4] = np.array([bits], dtype=np.uint64).view(np.float64)[0]
    assert np.isnan(covs[448, 4]) and np.isfinite(covs[:448]).all()
    guess = np.eye(4)
    assert gpu_ctx.set_robust(mt.NONE, 1.0, 1.0) == (mt.NONE, 1.0, 1.0)
    gpu_ctx.scan_upload(pts[:448], covs[:448])
    want = one_round(gpu_ctx, guess)
    assert want[27] == 448.0 and np.isfinite(want).all()
    assert np.array_equal(one_round(gpu_ctx, guess, capi.FLAG_NO_PERSISTENT), want)
    gpu_ctx.set_robust()
    gpu_ctx.scan_upload(pts, covs)
    before = gpu_ctx.counter(COUNTER_FALLBACKS)
    for flags in (capi.FLAG_NO_PERSISTENT, 0):
        r = gpu_ctx.align_resident(guess, 3, TSQ, COS, flags=flags, allow_degenerate=True)
        assert r.status == capi.ERR_DEGENERATE, (flags, r.status, r.message)
        assert (r.launches == 1) == (flags == 0)
        assert r.corr_count[0] == 449 and np.isnan(r.normal_eq[0]).any()
    assert gpu_ctx.counter(COUNTER_FALLBACKS) == before
    gpu_ctx.set_robust(mt.NONE, 1.0, 1.0)
    for flags in (capi.FLAG_NO_PERSISTENT, 0):
        got = one_round(gpu_ctx, guess, flags)
        assert got[27] == 448.0, (flags, got[27])
        assert np.isfinite(got).all(), (flags, got)
        assert np.array_equal(got, want), flags
    assert gpu_ctx.counter(COUNTER_FALLBACKS) == before
