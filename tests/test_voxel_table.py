"""The device voxel table on the tables ordinary data never makes: long probe chains, a chain that wraps from the
last slot to slot 0, tombstones inside chains, claims racing down one chain, and rehashes both ways.

The table (eskf_lio_amd/csrc) is open addressing with linear probing: slot = voxel_hash(key) & mask, states EMPTY /
LOCKED / FULL / TOMB.  Spatially coherent keys under the mixing hash make chains of one to three slots, so the keys
here are CRAFTED: `voxel_hash` below restates the hash in numpy (pinned to the compiled one on the CPU by
tests/native/voxel_hash.hip), and a family is a set of cells of a compact block of voxels whose home slot under the
largest mask a test reaches is one chosen slot.  Equal low bits under that mask mean equal low bits under every
smaller one, so the family collides in every table up to that size, and a test asserts the size it gets.

References: the oracle's LocalMap (`OracleMap`: insert, evict, match, align, export) and a plain dict for the mirror
calls (upsert, erase).  Keys, means, covariances and counts are compared with ==, poses to conftest's tolerances."""
import os
import subprocess

import numpy as np
import pytest

from conftest import POSE_TOL_M, POSE_TOL_RAD, TIGHT_POSE_TOL, pose_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the hash, restated -------------------------------------------------------------------------------------------
def fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def voxel_hash(keys):
    """voxel_hash (vgicp_device_fn.h) of N x 3 int32 keys -> N uint32, wrapping arithmetic as in C++."""
    k = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3).view(np.uint32)
    with np.errstate(over="ignore"):
        h = fmix32(k[:, 0] * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15))
        h = fmix32(h ^ (k[:, 1] * np.uint32(0x85EBCA77)))
        h = fmix32(h ^ (k[:, 2] * np.uint32(0xC2B2AE3D)))
    return h


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def predicted_slots(hint):
    """vgicp_map_reset: next_pow2(max(1024, 4 hint)) slots."""
    return next_pow2(max(1024, 4 * hint))


def test_numpy_hash_equals_the_compiled_hash(tmp_path):
    """tests/native/voxel_hash.hip, compiled by hipcc and run on the CPU (no device call), prints the table's hash of
    zero, small keys of both signs, the int32 edges in every position and 2000 pseudo-random keys: the restatement
    above must agree on every one, or the crafted families of the GPU tests would not collide."""
    exe = tmp_path / "voxel_hash"
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "voxel_hash.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-500:]
    rows = np.array([line.split() for line in run.stdout.splitlines()], dtype=np.int64)
    assert rows.shape[1] == 4 and rows.shape[0] >= 3000
    keys, want = rows[:, :3].astype(np.int32), rows[:, 3].astype(np.uint32)
    for edge in (0, -1, 2**31 - 1, -2**31):
        assert (keys == edge).any(axis=0).all(), edge           # every edge in every position
    assert np.array_equal(voxel_hash(keys), want)
    assert len(np.unique(want)) > 0.99 * len(np.unique(keys, axis=0))   # a hash, not a constant


# ---- crafted keys -------------------------------------------------------------------------------------------------
VOXEL = 0.3
ORIGIN = np.array([-217, -183, -13], dtype=np.int32)   # the block straddles 0 on every axis
BLOCK = (400, 400, 32)                                 # 5.1 M cells: ~310 per home slot under a 2^14-slot mask
CRAFT_SLOTS = 1 << 14                                  # the largest table any test here reaches
CRAFT_MASK = CRAFT_SLOTS - 1
FAMILY = 260                                           # keys per family: chains of at least 260 slots
HOME_A, HOME_B = 5_000, 9_000                          # B and B + 3 interleave; CRAFT_MASK wraps
_cells = {}


def block_cells():
    """Every cell of the block and its home slot under CRAFT_MASK (computed once)."""
    if not _cells:
        g = np.stack(np.meshgrid(*[np.arange(n) for n in BLOCK], indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
        g += ORIGIN
        _cells["keys"] = g
        _cells["home"] = voxel_hash(g) & np.uint32(CRAFT_MASK)
    return _cells["keys"], _cells["home"]


def family(home, count, seed):
    """`count` cells of the block whose home slot is `home`, and the rest of them (absent keys that share the home)."""
    keys, homes = block_cells()
    cand = keys[homes == home]
    assert len(cand) >= count + 20, (home, len(cand))
    cand = cand[np.random.default_rng(seed).permutation(len(cand))]
    return cand[:count], cand[count:]


def ordinary(count, seed, avoid):
    """`count` cells of the block at random, none of them a key of `avoid`."""
    keys, _ = block_cells()
    rng = np.random.default_rng(seed)
    taken = {tuple(k) for k in np.concatenate(avoid).tolist()}
    pick = keys[rng.choice(len(keys), count + len(taken) + 64, replace=False)]
    out = [k for k in pick.tolist() if tuple(k) not in taken][:count]
    assert len(out) == count
    return np.array(out, dtype=np.int32)


class Scene:
    """Four colliding families and ordinary voxels around them, each voxel with a mean inside its cell and an exactly
    symmetric covariance.  fam["slot"]: home HOME_A; fam["wrap"]: home CRAFT_MASK; fam["b"], fam["b3"]: homes HOME_B
    and HOME_B + 3, whose chains interleave."""

    def __init__(self, n_ordinary=3_000, seed=0):
        from eskf_lio_amd import synth
        self.fam, self.absent = {}, {}
        for i, (name, home) in enumerate((("slot", HOME_A), ("wrap", CRAFT_MASK), ("b", HOME_B), ("b3", HOME_B + 3))):
            self.fam[name], self.absent[name] = family(home, FAMILY if name in ("slot", "wrap") else 200, seed + i)
        self.ordinary = ordinary(n_ordinary, seed + 10, list(self.fam.values()) + list(self.absent.values()))
        self.keys = np.concatenate(list(self.fam.values()) + [self.ordinary])
        self.rng = np.random.default_rng(seed + 20)
        self.means, self.covs = self.payload(self.keys, seed)
        self.synth = synth

    def payload(self, keys, seed):
        from eskf_lio_amd import synth
        rng = np.random.default_rng(seed + 30)
        means = (keys.astype(np.float64) + rng.uniform(0.05, 0.95, size=keys.shape)) * VOXEL
        covs = synth.disc_covariances(seed + 40, 16, np.arange(len(keys), dtype=np.uint64))
        return means, covs

    def points_in(self, keys, per_voxel, seed, lo=0.02, hi=0.98):
        """per_voxel points inside every voxel of `keys` (away from the faces by `lo` / `hi` of a voxel)."""
        from eskf_lio_amd import synth
        rng = np.random.default_rng(seed)
        k = np.repeat(keys, per_voxel, axis=0)
        pts = (k.astype(np.float64) + rng.uniform(lo, hi, size=k.shape)) * VOXEL
        covs = synth.disc_covariances(seed + 1, 16, np.arange(len(k), dtype=np.uint64))
        return pts, covs


def check_chain(keys, mask, min_len=200):
    """The family's home slot under `mask` is one slot, and the family is long: a chain of >= min_len slots."""
    homes = np.unique(voxel_hash(keys) & np.uint32(mask))
    assert len(homes) == 1 and len(keys) >= min_len, (homes[:4], len(keys))
    return int(homes[0])


def mirror_export(d):
    """The dict mirror as map_export returns it: sorted by key, counts 1 (an upserted voxel starts at 1)."""
    keys = np.array(sorted(d), dtype=np.int32).reshape(-1, 3)
    keys = keys[np.lexsort(keys.T)]
    means = np.array([d[tuple(k)][0] for k in keys.tolist()]).reshape(-1, 3)
    covs = np.array([d[tuple(k)][1] for k in keys.tolist()]).reshape(-1, 9)
    return keys, means, covs, np.ones(len(keys), dtype=np.uint64)


def oracle_of(oracle, d, cap=1):
    """The oracle's LocalMap holding the dict mirror (each voxel built from its mean: mean, covariance, count 1)."""
    om = oracle.OracleMap(VOXEL, cap)
    if d:
        k, m, c, _ = mirror_export(d)
        om.insert(m, c)
    return om


def sorted_oracle_export(om):
    k, m, c, n = om.export()
    order = np.lexsort(k.T)
    return k[order], m[order], c[order], n[order]


def dict_of_oracle(om):
    k, m, c, n = om.export()
    assert (n == 1).all()
    return {tuple(kk): (mm, cc) for kk, mm, cc in zip(k.tolist(), m, c)}


def assert_export(got, want):
    assert len(got[0]) == len(want[0])
    assert len({tuple(k) for k in got[0].tolist()}) == len(got[0])       # no key twice
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def assert_match(ctx, om, pts, covs):
    got, ref = ctx.match(pts, covs), om.match(pts, covs)
    assert len(ref[4]) > 0
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    return len(ref[4])


def assert_align(ctx, om, pts, covs, guess, flags=0):
    from eskf_lio_amd import capi
    got = ctx.align(pts, covs, guess, 10, 1e-6, 2.0, flags=flags)
    ref = om.align(pts, covs, guess, 10, 1e-6, 2.0)
    assert got.iterations == ref.iterations and got.converged == ref.converged
    assert np.array_equal(got.corr_count, ref.corr_count)
    assert ref.corr_count.min() > 0
    dt, dr = pose_error(got.pose, ref.pose)
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and dt <= TIGHT_POSE_TOL and dr <= TIGHT_POSE_TOL
    if not flags & capi.FLAG_NO_PERSISTENT:
        assert got.launches == 1
    return got


def align_scan(scene, seed):
    """A scan near the families' and the ordinary voxels: two points per chain voxel, one per ordinary voxel, plus
    points in absent voxels that share the families' homes."""
    keys = np.concatenate(list(scene.fam.values()) * 2 + [scene.ordinary] + [a[:20] for a in scene.absent.values()])
    pts, covs = scene.points_in(keys, 1, seed, 0.1, 0.9)
    order = np.random.default_rng(seed).permutation(len(pts))
    return pts[order], covs[order]


GUESS_XI = [0.02, -0.015, 0.01, 2e-4, -3e-4, 4e-4]


def chained_table(ctx, scene):
    """The scene upserted in ONE shuffled batch into a 2^14-slot table; -> the dict mirror."""
    ctx.map_reset(VOXEL, CRAFT_SLOTS // 4)
    order = scene.rng.permutation(len(scene.keys))
    ctx.map_upsert(scene.keys[order], scene.means[order], scene.covs[order])
    assert ctx.map_size() == (len(scene.keys), predicted_slots(CRAFT_SLOTS // 4)) == (len(scene.keys), CRAFT_SLOTS)
    for name, keys in scene.fam.items():
        check_chain(keys, CRAFT_MASK)
    assert check_chain(scene.fam["wrap"], CRAFT_MASK) == CRAFT_MASK                 # this chain wraps to slot 0
    return {tuple(k): (m, c) for k, m, c in zip(scene.keys.tolist(), scene.means, scene.covs)}


def every_reader(ctx, om, d, scene, name, seed):
    """match, voxel_index, align (persistent and per-launch) and export of the table against the references."""
    from eskf_lio_amd import capi
    from oracle import binding
    fam, absent = scene.fam[name], scene.absent[name]
    keys = np.concatenate([fam, absent, scene.ordinary[:500]])
    pts, covs = scene.points_in(keys, 2, seed)
    assert assert_match(ctx, om, pts, covs) == 2 * sum(tuple(k) in d for k in keys.tolist())
    assert np.array_equal(ctx.voxel_index(pts), binding.voxel_index(VOXEL, pts))
    sp, sc = align_scan(scene, seed + 1)
    guess = scene.synth.se3_to_SE3(GUESS_XI)
    a = assert_align(ctx, om, sp, sc, guess)
    b = assert_align(ctx, om, sp, sc, guess, flags=capi.FLAG_NO_PERSISTENT)
    assert np.array_equal(a.corr_count, b.corr_count)
    assert ctx.counter(1) == 0
    assert_export(ctx.map_export(), mirror_export(d))


@pytest.mark.gpu
@pytest.mark.timeout(120)   # measured: 0.1 s each (and 0.3 s for the block's hashes, once)
@pytest.mark.parametrize("name", ["slot", "wrap"])
def test_chains_through_every_reader(gpu_ctx, oracle, name):
    """A colliding family (260 keys, one home slot; "wrap": home = the last slot, so the chain runs on at slot 0),
    two interleaving families and 3000 ordinary voxels, upserted in one shuffled batch: every voxel of the chain, the
    absent keys that share its home and the ordinary voxels are found (match), registered (align) and exported exactly
    as the references have them."""
    scene = Scene(seed=11)
    d = chained_table(gpu_ctx, scene)
    om = oracle_of(oracle, d)
    every_reader(gpu_ctx, om, d, scene, name, 100)


@pytest.mark.gpu
@pytest.mark.timeout(120)   # measured: 0.1 s each
@pytest.mark.parametrize("name", ["slot", "wrap"])
def test_tombstones_inside_chains(gpu_ctx, oracle, name):
    """Every other key of a chain erased in one batch (with absent keys sharing the home and duplicates): the
    survivors behind the tombstones are still found; the erased keys re-upserted with new values (and the survivors
    overwritten in the same batch) come back once, not twice; an eviction that cuts through the chain leaves what the
    reference's rule leaves; the rest of the chain erased in a later batch, through all those tombstones."""
    scene = Scene(seed=12)
    d = chained_table(gpu_ctx, scene)
    fam = scene.fam[name]
    gone, kept = fam[0::2], fam[1::2]
    batch = np.concatenate([gone, scene.absent[name][:30], gone[:10]])
    batch = batch[scene.rng.permutation(len(batch))]
    gpu_ctx.map_erase(batch)
    for k in gone.tolist():
        del d[tuple(k)]
    assert gpu_ctx.map_size() == (len(d), CRAFT_SLOTS)
    every_reader(gpu_ctx, oracle_of(oracle, d), d, scene, name, 200)

    # re-upsert: the erased keys get new values, the survivors behind the tombstones are overwritten
    back = np.concatenate([gone, kept])
    means, covs = scene.payload(back, 77)
    order = scene.rng.permutation(len(back))
    gpu_ctx.map_upsert(back[order], means[order], covs[order])
    for k, m, c in zip(back.tolist(), means, covs):
        d[tuple(k)] = (m, c)
    assert gpu_ctx.map_size() == (len(d), CRAFT_SLOTS)
    om = oracle_of(oracle, d)
    every_reader(gpu_ctx, om, d, scene, name, 300)

    # eviction through the chain: the threshold is the median distance of the family's voxel centres
    pos = np.array([1.1, -2.3, 0.4])
    centre = (fam.astype(np.float64) + 0.5) * VOXEL
    dist = np.sqrt(((centre - pos) ** 2).sum(axis=1))
    thr = float(np.median(dist)) + 1e-3
    removed = gpu_ctx.map_evict(pos, thr)
    assert removed == om.evict(pos, thr)
    d = dict_of_oracle(om)
    assert 0 < (dist > thr).sum() < len(fam) and gpu_ctx.map_size() == (len(d), CRAFT_SLOTS)
    every_reader(gpu_ctx, om, d, scene, name, 400)

    # erase whatever is left of the chain: every lookup walks past a dozen or more tombstones first
    rest = np.array([k for k in fam.tolist() if tuple(k) in d], dtype=np.int32)
    assert len(rest) > 50
    gpu_ctx.map_erase(rest)
    for k in rest.tolist():
        del d[tuple(k)]
    assert gpu_ctx.map_size() == (len(d), CRAFT_SLOTS)
    om = oracle_of(oracle, d)
    every_reader(gpu_ctx, om, d, scene, name, 500)


# ---- claims racing down one chain ---------------------------------------------------------------------------------
def race_scan(scene, seed):
    """Points of one insertion: many per absent chain voxel, several per present one, one to three per ordinary voxel
    (present and new), in scan order at random."""
    rng = np.random.default_rng(seed)
    parts = []
    for name in ("slot", "wrap"):
        fam = scene.fam[name]
        parts.append((fam[1::2], 12))                          # absent before the scan: every claim races
        parts.append((fam[0::4], 4))                           # present
    parts.append((scene.ordinary[:600], 2))
    parts.append((ordinary(400, seed, [scene.keys]), 3))
    pts, covs = [], []
    for i, (keys, per) in enumerate(parts):
        p, c = scene.points_in(keys, per, seed + 10 * i)
        pts.append(p)
        covs.append(c)
    pts, covs = np.concatenate(pts), np.concatenate(covs)
    order = rng.permutation(len(pts))
    return pts[order], covs[order]


def race_start(ctx, oracle, scene, cap):
    """Half of each colliding family present (built by an insertion, so that the reference has the same records),
    the ordinary voxels present; -> the oracle map."""
    ctx.map_reset(VOXEL, CRAFT_SLOTS // 4)
    om = oracle.OracleMap(VOXEL, cap)
    keys = np.concatenate([scene.fam["slot"][0::2], scene.fam["wrap"][0::2], scene.fam["b"], scene.fam["b3"],
                           scene.ordinary[:600]])
    p, c = scene.points_in(keys, 1, 900)
    new = ctx.map_insert_scan(p, c, np.eye(4), cap)
    om.insert(p, c)
    assert new == len(om) == len(keys) and ctx.map_size() == (len(keys), CRAFT_SLOTS)
    return om


@pytest.mark.gpu
@pytest.mark.timeout(120)   # measured: 0.02-0.06 s each
@pytest.mark.parametrize("path", ["scan", "resident", "resident_async"])
@pytest.mark.parametrize("cap", [1, 3, 1000])
def test_claim_races_down_a_chain(gpu_ctx, oracle, cap, path):
    """One insertion whose points fall in absent voxels of a 260-slot chain (12 points each: the claims race down the
    chain and wait on each other's LOCKED words), in present chain voxels, in the wrapping chain and in ordinary
    voxels, in scan order at random: the map equals the reference's serial loop bit for bit, and every voxel is then
    found where the lookups walk."""
    scene = Scene(seed=13)
    om = race_start(gpu_ctx, oracle, scene, cap)
    pts, covs = race_scan(scene, 31 + cap)
    before = len(om)
    om.insert(pts, covs)
    if path == "scan":
        assert gpu_ctx.map_insert_scan(pts, covs, np.eye(4), cap) == len(om) - before
    elif path == "resident":
        gpu_ctx.scan_upload(pts, covs)
        assert gpu_ctx.map_insert_resident(np.eye(4), cap) == len(om) - before
    else:
        gpu_ctx.scan_upload(pts, covs)
        gpu_ctx.map_insert_resident_async(np.eye(4), cap)
    assert gpu_ctx.map_size() == (len(om), CRAFT_SLOTS)
    got, ref = gpu_ctx.map_export(), sorted_oracle_export(om)
    assert_export(got, ref)
    assert ref[3].max() == min(cap, 12)
    p, c = scene.points_in(np.concatenate([scene.fam["slot"], scene.fam["wrap"], scene.absent["wrap"][:40]]), 1, 77)
    assert_match(gpu_ctx, om, p, c)


@pytest.mark.gpu
@pytest.mark.timeout(120)   # measured: 0.03 s each
@pytest.mark.parametrize("cap", [3, 1000])
def test_claim_races_down_a_chain_without_the_sort(oracle, cap):
    """The same races through the insertion that keeps scan order by per-voxel lists instead of a sort: a resident scan
    the device prepared itself (0.1 m grid under a 0.3 m map, as test_resident_insertion_without_the_sort_is_bit_exact
    sets up), dense around the voxels of both colliding chains."""
    from eskf_lio_amd import capi
    scene = Scene(seed=14)
    with capi.Context(0) as ctx:
        om = race_start(ctx, oracle, scene, cap)
        rng = np.random.default_rng(cap)
        for f, name in enumerate(("slot", "wrap")):
            keys = np.concatenate([scene.fam[name], scene.absent[name][:20], scene.ordinary[600 + 100 * f:700 + 100 * f]])
            k = np.repeat(keys, 10, axis=0)              # <= 10 kept points per map voxel: the table keeps its size
            raw = (k.astype(np.float64) + rng.uniform(0.0, 1.0, size=k.shape)) * VOXEL
            raw = raw[rng.permutation(len(raw))]
            kept, _ = ctx.scan_prepare(raw, None, None, None, 0.1, 30)
            gp, gc = ctx.scan_download()
            assert kept == len(gp) > len(keys)
            om.insert(gp, gc)
            if f == 0:
                ctx.map_insert_resident(np.eye(4), cap)
            else:
                ctx.map_insert_resident_async(np.eye(4), cap)
            assert ctx.map_size() == (len(om), CRAFT_SLOTS)
        got, ref = ctx.map_export(), sorted_oracle_export(om)
        assert_export(got, ref)
        assert ref[3].max() == 3 if cap == 3 else ref[3].max() > 3
        p, c = scene.points_in(np.concatenate([scene.fam["slot"], scene.fam["wrap"]]), 1, 78)
        assert_match(ctx, om, p, c)


# ---- rehashes -----------------------------------------------------------------------------------------------------
class TableModel:
    """ensure_table (vgicp_capi_memory.inl) restated: a call that may add `incoming` voxels first rebuilds the table
    when voxels + tombstones + incoming would fill more than half of it, into next_pow2(max(1024, 4 (voxels +
    incoming))) slots; the rebuild drops the tombstones.  Erase and evict turn voxels into tombstones."""

    def __init__(self, slots):
        self.voxels, self.tombs, self.slots = 0, 0, slots
        self.events = []

    def ensure(self, incoming):
        if (self.voxels + self.tombs + incoming) * 2 <= self.slots:
            return
        slots = next_pow2(max(1024, (self.voxels + incoming) * 4))
        self.events.append("grow" if slots > self.slots else "shrink" if slots < self.slots else "same")
        self.slots, self.tombs = slots, 0

    def remove(self, n):
        self.voxels -= n
        self.tombs += n


@pytest.mark.gpu
@pytest.mark.timeout(180)   # measured: 0.3 s
def test_churn_across_rehashes_both_ways(gpu_ctx, oracle):
    """Insert / evict / erase / upsert cycles over colliding and ordinary keys, the asynchronous insertion included.
    The test counts voxels and tombstones from the calls' results and predicts every rebuild from ensure_table's rule:
    after every call the map's size and slot count are the prediction and the export is the reference's.  On the way
    the table grows, shrinks after a mass eviction and is rebuilt at the same size by tombstones alone; the colliding
    families stay chains of >= 200 slots in every table up to 2^14 slots."""
    scene = Scene(n_ordinary=10_600, seed=15)
    colliding = np.concatenate([scene.fam["slot"], scene.fam["wrap"], scene.fam["b"], scene.fam["b3"]])
    pool = scene.ordinary
    rng = np.random.default_rng(5)
    model = TableModel(predicted_slots(0))
    gpu_ctx.map_reset(VOXEL, 0)
    d = {}

    def check():
        assert gpu_ctx.map_size() == (model.voxels, model.slots) == (len(d), model.slots)
        assert model.slots <= CRAFT_SLOTS
        for keys in scene.fam.values():
            check_chain(keys, model.slots - 1)
        assert_export(gpu_ctx.map_export(), mirror_export(d))

    def upsert(keys, seed):
        means, covs = scene.payload(keys, seed)
        order = rng.permutation(len(keys))
        model.ensure(len(keys))
        gpu_ctx.map_upsert(keys[order], means[order], covs[order])
        model.voxels += sum(tuple(k) not in d for k in keys.tolist())
        for k, m, c in zip(keys.tolist(), means, covs):
            d[tuple(k)] = (m, c)
        check()

    def erase(keys):
        model.remove(sum(tuple(k) in d for k in keys.tolist()))
        gpu_ctx.map_erase(keys)
        for k in keys.tolist():
            d.pop(tuple(k), None)
        check()

    def insert(keys, seed, resident_async=False):
        nonlocal d
        pts, covs = scene.points_in(keys, 2, seed)
        order = rng.permutation(len(pts))
        pts, covs = pts[order], covs[order]
        om = oracle_of(oracle, d)
        before = len(om)
        om.insert(pts, covs)
        model.ensure(len(pts))
        if resident_async:
            gpu_ctx.scan_upload(pts, covs)
            gpu_ctx.map_insert_resident_async(np.eye(4), 1)
        else:
            assert gpu_ctx.map_insert_scan(pts, covs, np.eye(4), 1) == len(om) - before
        model.voxels += len(om) - before
        d = dict_of_oracle(om)
        check()

    def evict(keep):
        """Evict around the block's centre, keeping about `keep` voxels."""
        nonlocal d
        pos = (ORIGIN + np.array(BLOCK) / 2.0) * VOXEL
        keys = np.array(sorted(d), dtype=np.int32)
        dist = np.sort(np.sqrt((((keys + 0.5) * VOXEL - pos) ** 2).sum(axis=1)))
        thr = float(0.5 * (dist[keep] + dist[keep - 1]))
        om = oracle_of(oracle, d)
        want = om.evict(pos, thr)
        assert gpu_ctx.map_evict(pos, thr) == want > 0
        model.remove(want)
        d = dict_of_oracle(om)
        check()

    check()
    upsert(colliding, 1)                          # 920 voxels into 1024 slots -> 4096
    insert(pool[:600], 2)                          # 1200 points may open voxels -> 16384
    erase(np.concatenate([colliding[0::3], pool[:200:2]]))
    insert(pool[600:1600], 3, resident_async=True)
    upsert(np.concatenate([colliding[0::3], pool[1600:2600]]), 4)
    for i in range(4):                             # fill the 2^14-slot table towards half with tombstones in it
        upsert(pool[2600 + 1000 * i:3600 + 1000 * i], 10 + i)
        erase(pool[2600 + 1000 * i:2600 + 1000 * i + 300])
    evict(800)                                     # mass eviction: most voxels become tombstones
    insert(np.concatenate([colliding[1::4], pool[7000:7300]]), 20)   # -> shrink
    for i in range(8):                             # erase / upsert at one size until tombstones alone force a rebuild
        live = np.array(sorted(d), dtype=np.int32)
        erase(live[rng.choice(len(live), 400, replace=False)])
        upsert(np.concatenate([colliding[i::8], pool[7300 + 400 * i:7700 + 400 * i]]), 30 + i)
    insert(np.concatenate([colliding[::2], pool[:200]]), 40, resident_async=True)
    assert "grow" in model.events and "shrink" in model.events and "same" in model.events, model.events


# ---- the other readers of a chained table -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(120)   # measured: 0.04-0.09 s each
@pytest.mark.parametrize("variant", ["dense", "many_points", "prefetch"])
def test_other_readers_of_a_chained_table(oracle, monkeypatch, variant):
    """The align of test_chains_through_every_reader through the launches that read the table differently: the dense
    copy of the FULL records (VGICP_DENSE_SLOTS=1; rebuilt after each mutation), several points per thread (a launch of
    two workgroups: memos, re-probed when a key changes), and one point per thread with every point within the prefetch
    margin of a face, so that the look-ahead probes the voxel behind it — chain voxels from both sides."""
    from eskf_lio_amd import capi
    scene = Scene(seed=16)
    env = {"dense": {"VGICP_PERSIST_GRID": "16", "VGICP_DENSE_SLOTS": "1"}, "many_points": {"VGICP_PERSIST_GRID": "2"},
           "prefetch": {}}[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with capi.Context(0) as ctx:
        for k in env:
            monkeypatch.delenv(k)
        d = chained_table(ctx, scene)
        guess = scene.synth.se3_to_SE3(GUESS_XI)
        if variant == "prefetch":
            # points 0.1-0.4 % of a voxel from a face shared by a chain voxel and its neighbour, on both sides
            rng = np.random.default_rng(3)
            fam = np.concatenate([scene.fam["slot"], scene.fam["wrap"]])
            axis = rng.integers(0, 3, len(fam))
            side = rng.integers(0, 2, len(fam))
            u = rng.uniform(0.1, 0.9, size=fam.shape)
            eps = rng.uniform(0.001, 0.004, len(fam))
            inside = np.where(side == 1, 1.0 - eps, eps)
            outside = np.where(side == 1, 1.0 + eps, -eps)
            a, b = u.copy(), u.copy()
            a[np.arange(len(fam)), axis] = inside
            b[np.arange(len(fam)), axis] = outside
            pts = np.concatenate([(fam + a) * VOXEL, (fam + b) * VOXEL, scene.points_in(scene.ordinary, 1, 5)[0]])
            covs = scene.synth.disc_covariances(9, 16, np.arange(len(pts), dtype=np.uint64))
            guess = scene.synth.se3_to_SE3([0.002, -0.001, 0.001, 0.0, 0.0, 1e-5])
        else:
            pts, covs = align_scan(scene, 7)
        om = oracle_of(oracle, d)
        assert_align(ctx, om, pts, covs, guess)
        if variant == "dense":
            # the copy is rebuilt after each kind of mutation
            gone = scene.fam["wrap"][0::2]
            ctx.map_erase(gone)
            for k in gone.tolist():
                del d[tuple(k)]
            om = oracle_of(oracle, d)
            assert_align(ctx, om, pts, covs, guess)
            means, covs2 = scene.payload(gone, 5)
            ctx.map_upsert(gone, means, covs2)
            for k, m, c in zip(gone.tolist(), means, covs2):
                d[tuple(k)] = (m, c)
            om = oracle_of(oracle, d)
            assert_align(ctx, om, pts, covs, guess)
        assert ctx.counter(1) == 0
        assert_export(ctx.map_export(), mirror_export(d))


@pytest.mark.gpu
@pytest.mark.timeout(120)   # measured: 0.07 s
def test_chained_table_on_two_sub_contexts(oracle):
    """A two-sub-context context (both on device 0) replicates the chained table: its export equals the single-device
    map bit for bit, before and after tombstones, and its align matches the reference."""
    from eskf_lio_amd import capi
    scene = Scene(seed=17)
    with capi.Context(0) as one, capi.Context([0, 0]) as two:
        d = chained_table(one, scene)
        chained_table(two, scene)
        assert_export(two.map_export(), one.map_export())
        gone = scene.fam["wrap"][1::2]
        one.map_erase(gone)
        two.map_erase(gone)
        for k in gone.tolist():
            del d[tuple(k)]
        assert two.map_size() == one.map_size() == (len(d), CRAFT_SLOTS)
        assert_export(two.map_export(), one.map_export())
        assert_export(one.map_export(), mirror_export(d))
        pts, covs = align_scan(scene, 8)
        om = oracle_of(oracle, d)
        assert_align(two, om, pts, covs, scene.synth.se3_to_SE3(GUESS_XI))
