"""tests/match_term_reference.py without a device: the 60-digit reference is right (against the oracle's per-term blocks
and against the Cramer form of tests/test_evaluate.py), a numpy restatement of the device's term in its operation order
stays inside the bound over the whole sweep with a factor of two to spare, six mutations of that restatement do not, and
every gated case of the weight test can be decided from the reference alone."""
import numpy as np
import pytest

import match_term_reference as mt

pytestmark = pytest.mark.skipif(mt.unavailable_reason() is not None, reason=str(mt.unavailable_reason()))

MUTATIONS = ("reciprocal 2^-26 off", "W transposed", "one sign of Q flipped", "slot (4, 3) from the upper triangle",
             "e = mu - p", "Huber without its correction step")
SLOPPY = 1.0 + 2.0 ** -26


def device_weight(kernel, c2, gate, raw, mutate=None):
    """robust_weight restated: d^2 = max(raw, 0); Cauchy c^2 x (1 / (c^2 + d^2)); Huber c^2 x rsq(c^2 d^2) beyond c^2."""
    d2 = max(raw, 0.0)
    w = 1.0
    if kernel == mt.CAUCHY:
        w = c2 * (1.0 / (c2 + d2))
    elif kernel == mt.HUBER and not d2 <= c2:
        rs = 1.0 / np.sqrt(c2 * d2)
        if mutate == MUTATIONS[5]:
            rs = rs * SLOPPY
        w = c2 * rs
    keep = not gate > 0.0 or raw <= gate
    return float(w) if keep else 0.0


def device_term(R, p, C9, mu, Cv9, mutate=None, robust=None):
    """accumulate_match (and evaluate_kernel's two spare slots) in fp64, operation for operation, without contraction:
    (29 values, count).  robust = (kernel, c, gate): the weighted row, its cost slot the raw residual."""
    R, C, S = [float(v) for v in mt.cm(R)], [float(v) for v in C9], [float(v) for v in Cv9]
    p, mu = [float(v) for v in p], [float(v) for v in mu]
    RC = [0.0] * 9
    for c in range(3):
        for r in range(3):
            RC[r + 3 * c] = R[r] * C[3 * c] + R[r + 3] * C[1 + 3 * c] + R[r + 6] * C[2 + 3 * c]
    for c in range(3):
        for r in range(3):
            S[r + 3 * c] += RC[r] * R[c] + RC[r + 3] * R[c + 3] + RC[r + 6] * R[c + 6]
    c00, c10, c20 = S[4] * S[8] - S[7] * S[5], S[5] * S[6] - S[8] * S[3], S[3] * S[7] - S[6] * S[4]
    det = c00 * S[0] + c10 * S[1] + c20 * S[2]
    inv = 1.0 / det
    if mutate == MUTATIONS[0]:
        inv = inv * SLOPPY
    c01, c11, c21 = S[7] * S[2] - S[1] * S[8], S[8] * S[0] - S[2] * S[6], S[6] * S[1] - S[0] * S[7]
    c02, c12, c22 = S[1] * S[5] - S[4] * S[2], S[2] * S[3] - S[5] * S[0], S[0] * S[4] - S[3] * S[1]
    W = [c00 * inv, c01 * inv, c02 * inv, c10 * inv, c11 * inv, c12 * inv, c20 * inv, c21 * inv, c22 * inv]
    if mutate == MUTATIONS[1]:
        W = [W[0], W[3], W[6], W[1], W[4], W[7], W[2], W[5], W[8]]
    e = [mu[k] - p[k] for k in range(3)] if mutate == MUTATIONS[4] else [p[k] - mu[k] for k in range(3)]
    g = [W[k] * e[0] + W[k + 3] * e[1] + W[k + 6] * e[2] for k in range(3)]
    raw = e[0] * g[0] + e[1] * g[1] + e[2] * g[2]
    count = 1.0
    if robust is not None:
        kernel, scale, gate = robust
        w = device_weight(kernel, scale * scale, gate, raw, mutate)
        count = 1.0 if w > 0.0 else 0.0
        W = [x * w if w > 0.0 else 0.0 for x in W]
    Q = [0.0] * 9
    for c in range(3):
        Q[0 + 3 * c] = p[1] * W[2 + 3 * c] - p[2] * W[1 + 3 * c]
        Q[1 + 3 * c] = p[2] * W[0 + 3 * c] - p[0] * W[2 + 3 * c]
        Q[2 + 3 * c] = p[0] * W[1 + 3 * c] - p[1] * W[0 + 3 * c]
    if mutate == MUTATIONS[2]:
        Q[7] = p[2] * W[6] + p[0] * W[8]
    v = [0.0] * 29
    v[0], v[1], v[2], v[3], v[4], v[5] = W[0], W[1], W[4], W[2], W[5], W[8]
    for r in range(3):
        base = (3 + r) * (4 + r) // 2
        q0, q1, q2 = Q[r], Q[r + 3], Q[r + 6]
        v[base], v[base + 1], v[base + 2] = q0, q1, q2
        v[base + 3] = q2 * p[1] - q1 * p[2]
        if r >= 1:
            v[base + 4] = q0 * p[2] - q2 * p[0]
        if r >= 2:
            v[base + 5] = q1 * p[0] - q0 * p[1]
    if mutate == MUTATIONS[3]:
        v[13] = Q[0] * p[2] - Q[6] * p[0]              # J^T W J (3, 4) where (4, 3) belongs
    for k in range(3):
        v[21 + k] = W[k] * e[0] + W[k + 3] * e[1] + W[k + 6] * e[2]
        v[24 + k] = Q[k] * e[0] + Q[k + 3] * e[1] + Q[k + 6] * e[2]
    v[27] = raw
    v[28] = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    return np.array(v), count


@pytest.fixture(scope="module")
def swept():
    vmap, groups = mt.sweep()
    return vmap, groups, mt.references()


def restated(vmap, g, c, mutate=None, robust=None):
    return device_term(c.R, c.p, g.C9, vmap.means[c.voxel], vmap.covs[c.voxel], mutate, robust)


def test_the_sweep_is_what_it_says(swept, oracle):
    """About 60 voxels, about 40 groups, no group over 64 poses; p is oracle.transform's, bit for bit, and lies in the
    voxel the case names; every axis of the docstring is there, with the values it names."""
    vmap, groups, refs = swept
    assert 48 <= len(vmap.keys) <= 72 and len(set(vmap.keys)) == len(vmap.keys)
    everything = groups + mt.weight_groups()
    assert 36 <= len(everything) <= 48 and all(1 <= len(g.cases) <= 64 for g in groups)
    for g in everything:
        for c in g.cases:
            tp, _ = oracle.transform(g.x[None], g.C9[None], c.pose)
            assert np.array_equal(tp[0], c.p), (g.name, c.label)
            assert tuple(oracle.voxel_index(mt.VOXEL, c.p[None])[0]) == vmap.keys[c.voxel], (g.name, c.label)
    by_axis = {}
    for g in groups:
        by_axis.setdefault(g.axis, []).append(g)
    assert set(by_axis) == {"scale", "conditioning", "indefinite", "asymmetry", "distance", "anchor"}
    assert all(len(v) >= 2 for v in by_axis.values())
    for g in by_axis["conditioning"]:
        rho = np.array([refs[(g.name, k)].rho for k in range(len(g.cases))])
        assert np.allclose(rho, mt.DECADES, rtol=1e-3), (g.name, rho)
    small = {g.name: refs[(g.name, 10)].l for g in by_axis["conditioning"]}
    assert all((l[1] > 0.5) == ("one small" in name) for name, l in small.items())
    for g in by_axis["indefinite"]:
        for k, c in enumerate(g.cases):
            t = refs[(g.name, k)]
            lam = float(c.label.split(",")[0].split()[-1])
            assert abs(t.l[2] / abs(lam) - 1.0) < 1e-6, (c.label, t.l)
            assert (t.raw < 0) == (lam < 0 and "along" in c.label), (c.label, t.raw)
    for g in by_axis["asymmetry"]:
        C = mt.from_cm(g.C9)
        assert C[0, 1] != C[1, 0] and np.array_equal(np.triu(C, 1)[[0, 1], [2, 2]], np.tril(C, -1)[[2, 2], [0, 1]])
    for g in by_axis["distance"]:
        norms = [np.linalg.norm(c.p) for c in g.cases]
        want = float(g.name.split()[-1])
        assert all(abs(n - want) <= 0.15 * max(want, 1e-300) for n in norms), (g.name, norms)
        if want > 0:
            e = np.array([np.linalg.norm(c.p - vmap.means[c.voxel]) for c in g.cases])
            assert (e == 0.0).any() and ((e > 0) & (e < 1e-8)).any() and np.isclose(e, 0.1).any() and np.isclose(e, 1.0).any()


def test_reference_against_the_oracle_blocks(swept, oracle):
    """oracle.jtj_jtr (ICP::computeJTJAndJTr restated, fp64) on S = oracle.transform's covariance + C_voxel, over the
    whole sweep with the asymmetric and the indefinite groups: the lower triangle of its 6 x 6 and its J^T r within the
    reference's bound (the oracle performs the device's operations in another order; the same count covers it).  The
    UPPER triangle of the oracle's block equals the lower one's transpose only where W is symmetric: in the asymmetry
    groups the reference's slot (4, 3) is nearer to the oracle's (4, 3) than to its (3, 4)."""
    vmap, groups, refs = swept
    worst = {}
    for g in groups:
        for k, c in enumerate(g.cases):
            t = refs[(g.name, k)]
            _, tc = oracle.transform(g.x[None], g.C9[None], c.pose)
            S = mt.from_cm(tc[0]) + mt.from_cm(vmap.covs[c.voxel])
            JTJ, JTr = oracle.jtj_jtr(c.p, vmap.means[c.voxel], S)
            got = np.array([JTJ[r, col] for r, col in mt.SLOTS] + list(JTr))
            ratio = t.differences(np.r_[got, t.f64[27:]])[:27] / np.where(t.bounds()[:27] > 0, t.bounds()[:27], 1.0)
            if g.exact:
                assert np.array_equal(got, t.f64[:27]), (g.name, c.label)
            assert (ratio <= 1.0).all(), (g.name, c.label, ratio)
            worst[g.name] = max(worst.get(g.name, 0.0), ratio.max())
            if g.axis == "asymmetry" and g.name.endswith("0.7"):
                assert abs(JTJ[4, 3] - t.f64[13]) < abs(JTJ[3, 4] - t.f64[13])
    for name, ratio in worst.items():
        print(f"{name}: the oracle's worst |difference| / bound {ratio:.3e}")


def test_reference_against_the_cramer_form(swept, oracle):
    """test_evaluate.reference_sums (extended precision, Cramer's rule, on the oracle's fp64 transformed covariance) for
    every swept case with kappa <= 100 whose voxel mean lies in its own cell (an oracle map files a voxel under its
    mean's key): count 1, cost and |e|^2 within the bound."""
    from test_evaluate import reference_sums
    vmap, groups, refs = swept
    keys, means, covs = vmap.arrays()
    inside = np.array([tuple(k) == tuple(np.floor(m / mt.VOXEL).astype(int)) for k, m in zip(keys, means)])
    om = oracle.OracleMap(mt.VOXEL, 1)
    om.insert(means[inside], covs[inside])
    assert len(om) == int(inside.sum())
    done, worst = 0, 0.0
    for g in groups:
        for k, c in enumerate(g.cases):
            t = refs[(g.name, k)]
            if not inside[c.voxel] or t.l[0] / t.l[2] > 100.0:
                continue
            m, cost, sq, kappa = reference_sums(oracle, om, g.x[None], g.C9[None], c.pose)
            d = t.differences(np.r_[t.f64[:27], cost, sq])[27:]
            assert m == 1 and d[0] <= t.bounds()[27] and d[1] <= t.bounds()[28], (g.name, c.label, d, t.bounds()[27:])
            worst = max(worst, d[0] / t.bounds()[27] if t.bounds()[27] else 0.0)
            done += 1
    print(f"{done} cases with kappa <= 100; worst cost |difference| / bound {worst:.3e}")
    assert done >= 200


def sweep_ratios(vmap, groups, refs, mutate=None):
    """{group: worst |restatement - reference| / bound over its cases and the 29 values} and whether an exact group's
    values are the reference's."""
    worst, exact_ok = {}, {}
    for g in groups:
        for k, c in enumerate(g.cases):
            t = refs[(g.name, k)]
            got, count = restated(vmap, g, c, mutate)
            assert count == 1.0
            b = t.bounds()
            ratio = t.differences(got) / np.where(b > 0, b, 1.0)
            ratio[(b == 0) & (t.differences(got) > 0)] = np.inf
            worst[g.name] = max(worst.get(g.name, 0.0), float(ratio.max()))
            if g.exact:
                exact_ok[g.name] = exact_ok.get(g.name, True) and np.array_equal(got, t.f64)
    return worst, exact_ok


def test_the_restatement_stays_inside_the_bound(swept):
    """The device's term in numpy, in its operation order without contraction: every one of the 29 values of every swept
    case within HALF its bound, the anchors equal; worst ratio per group printed."""
    vmap, groups, refs = swept
    worst, exact_ok = sweep_ratios(vmap, groups, refs)
    for name, ratio in worst.items():
        print(f"{name}: worst |restatement - reference| / bound {ratio:.3e}")
    assert max(worst.values()) <= 0.5, worst
    assert exact_ok and all(exact_ok.values()), exact_ok


@pytest.mark.parametrize("mutation", MUTATIONS[:5])
def test_a_mutated_term_leaves_the_bound(swept, mutation):
    """Each mutation exceeds the bound somewhere in the sweep and fails an exact anchor (W transposed and the slot from
    the upper triangle: the shear anchor, whose W is not symmetric; the others: both)."""
    vmap, groups, refs = swept
    worst, exact_ok = sweep_ratios(vmap, groups, refs, mutation)
    over = {name: r for name, r in worst.items() if r > 1.0}
    print(f"{mutation}: over the bound in {len(over)} of {len(worst)} groups, worst ratio {max(worst.values()):.3e}; "
          f"anchors still equal: {[n for n, ok in exact_ok.items() if ok]}")
    assert over, worst
    assert not exact_ok["anchor: S a shear"]
    if mutation not in (MUTATIONS[1], MUTATIONS[3]):
        assert not exact_ok["anchor: S a diagonal of powers of two"]


def weight_ratios(vmap, mutate=None):
    """Over weight_groups(): (worst |weighted restatement - w_ref x reference| / bound per group, counts all equal the
    reference's, the exactly representable rows of the exact groups all equal, how many of those there are)."""
    worst, counts_ok, exact_ok, exact = {}, True, True, 0
    for g in mt.weight_groups():
        for c in g.cases:
            t = mt.term(c.R, c.p, g.C9, vmap.means[c.voxel], vmap.covs[c.voxel])
            row = mt.weighted_row(t, *g.robust)
            got, count = restated(vmap, g, c, mutate, g.robust)
            counts_ok = counts_ok and (count == 1.0) == row.counted
            if g.exact and row.representable:
                exact += 1
                exact_ok = exact_ok and np.array_equal(got[:27], [float(v) for v in row.values])
            worst[g.name] = max(worst.get(g.name, 0.0), float(row.ratios(got[:27]).max()))
    return worst, counts_ok, exact_ok, exact


def test_the_weighted_restatement_and_its_mutation(swept):
    """robust_weight restated (IEEE 1 / x and 1 / sqrt(x) for the device's v_rcp_f64 / v_rsq_f64 + one step): every weighted
    slot within half of w_ref x (the plain bound) + 4 u of w_ref x (the reference slot), every count (w_ref > 0), and ==
    wherever the weight and its 27 products are fp64 numbers (S = I: 24 of the 32 exact cases; Cauchy's 1 / 5 and
    4 / 5 and the weights of e = 1 + 2^-52 are not).  Huber's reciprocal square root without its correction step —
    y (1 + 2^-26) — leaves the bound in every Huber group and fails an exact case (e = (2, 0, 0), c = 1: w = 1 / 2)."""
    vmap, _, _ = swept
    worst, counts_ok, exact_ok, exact = weight_ratios(vmap)
    for name, ratio in worst.items():
        print(f"{name}: worst |weighted restatement - reference| / bound {ratio:.3e}")
    print(f"{exact} exactly representable rows")
    assert counts_ok and exact_ok and exact >= 20 and max(worst.values()) <= 0.5, worst
    worst, counts_ok, exact_ok, _ = weight_ratios(vmap, MUTATIONS[5])
    huber = {n: r for n, r in worst.items() if f"sweep {mt.HUBER} " in n}
    print(f"{MUTATIONS[5]}: worst ratio per Huber group {huber}")
    assert counts_ok and not exact_ok and len(huber) == 2 and all(r > 1.0 for r in huber.values()), worst


def test_gate_cases_are_decidable(swept):
    """No case that runs under a gate has its reference residual within the residual's bound of the gate, so count 0 or 1
    follows from the reference alone for every gated case: none is left out.  The bound of the exact cases (S = I, e
    along x: every operation exact but the one product e0 x e0) is one rounding, u |raw| — asserted: the restatement
    returns the correctly rounded residual — and zero where the residual is an fp64 number: e = (1, 0, 0) meets the gate
    1.0 itself and is kept, 1 + 2^-52 (4 u beyond it) is not."""
    vmap, _, _ = swept
    gated = undecided = 0
    nearest = np.inf
    for g in mt.weight_groups():
        kernel, c, gate = g.robust
        if not gate > 0.0:
            continue
        for case in g.cases:
            t = mt.term(case.R, case.p, g.C9, vmap.means[case.voxel], vmap.covs[case.voxel])
            gated += 1
            gap = abs(float(t.raw - mt.mpf(gate)))
            bound = t.bounds()[27]
            if g.exact:
                got, _ = restated(vmap, g, case)
                assert got[27] == float(t.raw), (g.name, case.label)
                bound = 0.0 if mt.mpf(float(t.raw)) == t.raw else mt.U * abs(float(t.raw))
                undecided += gap <= bound and gap != 0.0
                continue
            nearest = min(nearest, gap / bound)
            undecided += gap <= bound
    print(f"{gated} gated cases, {undecided} undecided; the nearest lies {nearest:.3e} bounds from its gate")
    assert gated > 100 and undecided == 0


def test_exact_weight_cases_are_what_they_say(swept):
    vmap, _, _ = swept
    for g in mt.weight_groups():
        if not g.exact:
            continue
        e = {c.label: c.p - vmap.means[c.voxel] for c in g.cases}
        assert np.array_equal(e["unit e 1"], [1.0, 0.0, 0.0]) and np.array_equal(e["unit e 2"], [2.0, 0.0, 0.0])
        assert np.array_equal(e["unit e 0"], [0.0, 0.0, 0.0]) and np.array_equal(e["unit e 1 + 2^-52"], [1.0 + 2.0 ** -52, 0.0, 0.0])
