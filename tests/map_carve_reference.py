"""The reference of the free-space carving tests (include/vgicp_hip_map_carve.h): the header's rule restated operation by
operation in numpy (float64 ufuncs round every product, sum, quotient and square root once and fuse nothing, which is
what the rule asks), the brute-force sandwich that does not depend on the order of those operations, and the scenes both
test files build.  Not a test module; tests/test_map_carve_cpu.py checks the reference on its own, tests/test_map_carve.py
holds the device against it."""
from dataclasses import dataclass

import numpy as np

from eskf_lio_amd import synth

KEY_LIMIT = float(2 ** 30)
MAX_STEPS = 4096          # VGICP_CARVE_MAX_STEPS

VOXEL = 0.5
MAP_VOXELS = 20_000
SIZES = (1, 63, 64, 65, 1_000, 3_000)
MIN_HITS = (1, 2, 5)
STRIDES = (1, 3)
MARGINS = (0.0, VOXEL)
ORIGIN = (0.11, -0.07, 0.23)
MAX_RANGE = 60.0
SCENE_SEEDS = (11, 12)    # the committed seeds: test_map_carve_cpu.py shows the sandwich is tight on them


@dataclass
class Params:
    margin: float = 0.0
    max_range: float = MAX_RANGE
    min_hits: int = 1
    stride: int = 1
    origin: tuple = (0.0, 0.0, 0.0)

    def as_dict(self):
        return dict(margin=self.margin, max_range=self.max_range, min_hits=self.min_hits, stride=self.stride,
                    origin=self.origin)


def transform(T, pts):
    """x |-> ((R[.,0] x0 + R[.,1] x1) + R[.,2] x2) + t, the insertion's transform_point."""
    T = np.asarray(T, dtype=np.float64)
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def keys_of(x, h):
    """floor(x / h) per axis -> (int64 keys, defined): defined iff all three lie within +-2^30."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(x / h)
        ok = np.all(np.abs(q) <= KEY_LIMIT, axis=1)
    return np.where(ok[:, None], q, 0.0).astype(np.int64), ok


def boundary(k, d, o, h):
    """The parameter at which the ray leaves voxel k along one axis: +inf where d == 0."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = ((k + (d > 0.0)).astype(np.float64) * h - o) / d
    return np.where(d == 0.0, np.inf, t)


def rays_of(pts, T, p: Params):
    """What the ray rule makes of every point: (e, o, d, length, t_stop, casts)."""
    e = transform(T, pts)
    o = transform(T, np.asarray(p.origin, dtype=np.float64))[0]
    d = e - o
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        shorter = length - p.margin
        t_stop = np.where(shorter < p.max_range, shorter, p.max_range) / length
        casts = (np.arange(len(e)) % p.stride == 0) & (t_stop > 0.0) & np.all(np.isfinite(d), axis=1)
    return e, o, d, length, t_stop, casts


def walk(pts, T, voxel, p: Params):
    """The traversal of every ray in lockstep -> (ray index of every visit, its key (m, 3) int64, steps per point, e)."""
    h = float(voxel)
    e, o, d, length, t_stop, casts = rays_of(pts, T, p)
    k0, o_defined = keys_of(o[None, :], h)
    if not o_defined[0]:
        casts[:] = False
    ray = np.flatnonzero(casts)
    k = np.repeat(k0, len(ray), axis=0)
    dd, ts = d[ray], t_stop[ray]
    with np.errstate(invalid="ignore", over="ignore"):
        cells = np.ceil((ts * length[ray]) / h)
    cells = np.where(cells <= MAX_STEPS + 1.0, cells, MAX_STEPS + 1.0)
    max_steps = 3 * cells.astype(np.int64) + 3
    sgn = np.where(dd > 0.0, 1, -1).astype(np.int64)
    tmax = np.stack([boundary(k[:, a], dd[:, a], o[a], h) for a in range(3)], axis=1)
    visit_ray, visit_key = [ray.copy()], [k.copy()]
    steps = np.zeros(len(pts), dtype=np.int64)
    steps[ray] = 1
    alive = np.arange(len(ray))
    step = 0
    while len(alive):
        tx, ty, tz = tmax[alive, 0], tmax[alive, 1], tmax[alive, 2]
        axis = np.where((tx <= ty) & (tx <= tz), 0, np.where(ty <= tz, 1, 2))
        t_in = tmax[alive, axis]
        go = (t_in < ts[alive]) & (step < max_steps[alive])
        alive, axis = alive[go], axis[go]
        if not len(alive):
            break
        k[alive, axis] += sgn[alive, axis]
        for a in range(3):
            sel = alive[axis == a]
            tmax[sel, a] = boundary(k[sel, a], dd[sel, a], o[a], h)
        visit_ray.append(ray[alive])
        visit_key.append(k[alive].copy())
        steps[ray[alive]] += 1
        step += 1
    return np.concatenate(visit_ray), np.concatenate(visit_key), steps, e


def match(map_keys, query_keys):
    """Index into map_keys of every query key, or -1 (exact, any int64 keys)."""
    m = len(map_keys)
    if m == 0 or len(query_keys) == 0:
        return np.full(len(query_keys), -1, dtype=np.int64)
    both = np.concatenate([np.asarray(map_keys, dtype=np.int64), np.asarray(query_keys, dtype=np.int64)])
    _, inverse = np.unique(both, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    where = np.full(inverse.max() + 1, -1, dtype=np.int64)
    where[inverse[:m]] = np.arange(m)
    return where[inverse[m:]]


@dataclass
class Result:
    hits: np.ndarray        # per map voxel: distinct rays that visit it
    shield: np.ndarray      # per map voxel, bool
    removed: np.ndarray     # per map voxel, bool
    rays: int
    visits: int
    steps: np.ndarray       # per point: voxels its ray visits (0: no ray)

    @property
    def touched(self):
        return int(np.count_nonzero(self.hits >= 1))

    @property
    def shielded(self):
        return int(np.count_nonzero((self.hits >= 1) & self.shield))

    def counts(self):
        return dict(rays=self.rays, visits=self.visits, touched=self.touched, shielded=self.shielded,
                    removed=int(self.removed.sum()))


def carve(map_keys, voxel, pts, T, p: Params) -> Result:
    """The rule on a map given by the keys of its FULL voxels (distinct rows)."""
    map_keys = np.asarray(map_keys, dtype=np.int64).reshape(-1, 3)
    visit_ray, visit_key, steps, e = walk(pts, T, voxel, p)
    hits = np.zeros(len(map_keys), dtype=np.int64)
    at = match(map_keys, visit_key)
    np.add.at(hits, at[at >= 0], 1)
    ek, defined = keys_of(e, float(voxel))
    sat = match(map_keys, ek[defined])
    shield = np.zeros(len(map_keys), dtype=bool)
    shield[sat[sat >= 0]] = True
    removed = (hits >= p.min_hits) & ~shield
    return Result(hits, shield, removed, int(np.count_nonzero(steps)), int(len(visit_ray)), steps)


def sorted_keys(keys):
    keys = np.asarray(keys).reshape(-1, 3)
    return keys[np.lexsort(keys.T)] if len(keys) else keys


# ---- the sandwich: independent of the order of the rule's operations -------------------------------------------------
def slab_counts(map_keys, voxel, pts, T, p: Params, eps_factor=1e-7, chunk=64):
    """Brute force over every (ray, voxel) pair: the segment o + s d, s in [0, t_stop -+ eps / len], against the voxel's
    box shrunk / grown by eps = eps_factor * voxel -> (certain count, possible count) per voxel."""
    h = float(voxel)
    eps = eps_factor * h
    e, o, d, length, t_stop, casts = rays_of(pts, T, p)
    lo = np.asarray(map_keys, dtype=np.float64).reshape(-1, 3) * h
    hi = lo + h
    certain = np.zeros(len(lo), dtype=np.int64)
    possible = np.zeros(len(lo), dtype=np.int64)
    ray = np.flatnonzero(casts)

    def crossed(idx, lo_b, hi_b, s_end):
        dd = d[idx][:, None, :]                                  # (r, 1, 3)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = (lo_b[None, :, :] - o) / dd
            t2 = (hi_b[None, :, :] - o) / dd
        inside = (o >= lo_b[None, :, :]) & (o <= hi_b[None, :, :])   # an axis the ray does not move along
        flat = dd == 0.0
        t_near = np.where(flat, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
        t_far = np.where(flat, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
        enter = np.maximum(t_near.max(axis=2), 0.0)
        leave = np.minimum(t_far.min(axis=2), s_end[:, None])
        return enter <= leave

    for at in range(0, len(ray), chunk):
        idx = ray[at:at + chunk]
        cut = eps / length[idx]
        certain += crossed(idx, lo + eps, hi - eps, t_stop[idx] - cut).sum(axis=0)
        possible += crossed(idx, lo - eps, hi + eps, t_stop[idx] + cut).sum(axis=0)
    return certain, possible


def check_sandwich(removed_mask, shield, certain, possible, min_hits):
    """Every unshielded voxel with certain >= min_hits is removed; every removed voxel is unshielded with possible >=
    min_hits.  -> the two lists of offenders (both must be empty)."""
    must = (certain >= min_hits) & ~shield
    may = (possible >= min_hits) & ~shield
    return np.flatnonzero(must & ~removed_mask), np.flatnonzero(removed_mask & ~may)


# ---- scenes ---------------------------------------------------------------------------------------------------------
def scene_pose():
    return synth.se3_to_SE3((0.8, -0.5, 0.3, 0.02, -0.03, 0.6))


def make_scene(n, seed=SCENE_SEEDS[0], vmap=None):
    """A scan of n points around the sensor (frame of the scan; origin ORIGIN): two thirds inside the map's cube, a third
    up to ~60 m away, so that rays cross the whole cube and leave it.  -> (map, points, pose)."""
    vmap = vmap if vmap is not None else synth.make_map(MAP_VOXELS, voxel_size=VOXEL)
    idx = np.arange(n, dtype=np.uint64)
    u = [synth.rand_unit(seed, 300 + k, idx) for k in range(4)]
    span = vmap.hi - vmap.lo
    pts = np.stack([vmap.lo + span * u[a] for a in range(3)], axis=1)
    far = u[3] < 1.0 / 3.0
    pts = np.where(far[:, None], pts * (2.0 + 12.0 * u[3][:, None]), pts)
    return vmap, np.ascontiguousarray(pts), scene_pose()
