"""The reference of the ray-report tests (include/vgicp_hip_map_rays.h): the header's rule restated operation by operation
in numpy (float64 ufuncs round every product, sum, quotient and square root once and fuse nothing, which is what the
rule asks) on free-space carving's pieces (tests/map_carve_reference.py: one definition of the step serves both), a
brute-force first hit that does not depend on the order of those operations, and the scene both test files build.
Not a test module; tests/test_map_rays_cpu.py checks the reference on its own, tests/test_map_rays.py holds the device
against it."""
from dataclasses import dataclass

import numpy as np

from eskf_lio_amd import synth
from map_carve_reference import MAX_STEPS, boundary, keys_of, match, scene_pose, transform  # noqa: F401

NO_RAY, OPEN, OWN, BEHIND, CONFIRMED, BLOCKED, NEAR = range(7)
NO_HIT_RANGE_BITS = 0x7FF8000000000000
NO_HIT_KEY = -2 ** 31

VOXEL = 0.5
SHELL = 24                # the room: a one-voxel shell at max|k| = SHELL
WINDOW = 4                # a (2 WINDOW + 1)^2 window cut out of the +x wall
STALE = 240               # stale voxels inside the room, 3 - 8 m from the sensor
SIZES = (1, 63, 64, 65, 1_000, 3_000)
STRIDES = (1, 3)
MARGIN_BEYOND = ((0.0, 0.0), (1.0, 20.0))
ORIGIN = (0.11, -0.07, 0.23)
MAX_RANGE = 60.0
SCENE_SEEDS = (21, 22)    # the committed seeds: test_map_rays_cpu.py shows every class is populated on them
DIRECTION_STREAM = 320    # of the random directions: with it both seeds put a ray into every class at n = 63, stride 3


@dataclass
class Params:
    margin: float = 0.0
    beyond: float = 0.0
    max_range: float = MAX_RANGE
    stride: int = 1
    origin: tuple = (0.0, 0.0, 0.0)

    def as_dict(self):
        return dict(margin=self.margin, beyond=self.beyond, max_range=self.max_range, stride=self.stride, origin=self.origin)


class Lookup:
    """Index into map_keys of a batch of keys, or -1.  Keys within +-2^20 (every scene of the tests) go through one
    sorted int64 code; anything else through map_carve_reference.match."""
    LIMIT = 1 << 20

    def __init__(self, map_keys):
        self.keys = np.asarray(map_keys, dtype=np.int64).reshape(-1, 3)
        self.fast = len(self.keys) > 0 and bool(np.all(np.abs(self.keys) < self.LIMIT))
        if self.fast:
            code = self.code(self.keys)
            self.order = np.argsort(code, kind="stable")
            self.sorted = code[self.order]

    @classmethod
    def code(cls, k):
        return ((k[:, 0] + cls.LIMIT) << 42) | ((k[:, 1] + cls.LIMIT) << 21) | (k[:, 2] + cls.LIMIT)

    def __call__(self, query):
        query = np.asarray(query, dtype=np.int64).reshape(-1, 3)
        if not self.fast:
            return match(self.keys, query)
        out = np.full(len(query), -1, dtype=np.int64)
        inside = np.all(np.abs(query) < self.LIMIT, axis=1)
        code = self.code(query[inside])
        at = np.minimum(np.searchsorted(self.sorted, code), len(self.sorted) - 1)
        out[inside] = np.where(self.sorted[at] == code, self.order[at], -1)
        return out


def rays_of(pts, T, p: Params):
    """What the ray rule makes of every point: (e, o, d, length, t_end, t_front, casts) — key(o) not asked yet."""
    e = transform(T, pts)
    o = transform(T, np.asarray(p.origin, dtype=np.float64))[0]
    d = e - o
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        longer = length + p.beyond
        t_end = np.where(longer < p.max_range, longer, p.max_range) / length
        t_front = (length - p.margin) / length
        casts = (np.arange(len(e)) % p.stride == 0) & (length > 0.0) & (t_end > 0.0) & np.all(np.isfinite(d), axis=1)
    return e, o, d, length, t_end, t_front, casts


@dataclass
class Result:
    status: np.ndarray      # uint8 (n)
    range: np.ndarray       # float64 (n): t_in * len, the NaN pattern NO_HIT_RANGE_BITS with no hit
    hit_key: np.ndarray     # int32 (n, 3): NO_HIT_KEY with no hit
    steps: np.ndarray       # uint32 (n): voxels visited, 0 with no ray
    hit: np.ndarray         # int64 (n): index into map_keys of the hit, -1 with none
    visit_ray: np.ndarray   # every visit in step order: the point ...
    visit_key: np.ndarray   # ... and the key (m, 3) int64

    def counts(self):
        return dict(rays=int(np.count_nonzero(self.status != NO_RAY)), visits=int(self.steps.sum()),
                    by_class=[int(np.count_nonzero(self.status == c)) for c in range(8)])


def rays(map_keys, voxel, pts, T, p: Params) -> Result:
    """The rule on a map given by the keys of its FULL voxels (distinct rows)."""
    h = float(voxel)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    find = Lookup(map_keys)
    e, o, d, length, t_end, t_front, casts = rays_of(pts, T, p)
    # CONFIRM: every point, whatever the stride
    ek, e_defined = keys_of(e, h)
    confirmed = np.zeros(len(find.keys), dtype=bool)
    own_voxel = find(ek[e_defined])
    confirmed[own_voxel[own_voxel >= 0]] = True
    # RAY
    k0, o_defined = keys_of(o[None, :], h)
    if not o_defined[0]:
        casts[:] = False
    ray = np.flatnonzero(casts)
    k = np.repeat(k0, len(ray), axis=0)
    dd, te = d[ray], t_end[ray]
    with np.errstate(invalid="ignore", over="ignore"):
        cells = np.ceil((te * length[ray]) / h)
    cells = np.where(cells <= MAX_STEPS + 1.0, cells, MAX_STEPS + 1.0)
    max_steps = 3 * cells.astype(np.int64) + 3
    sgn = np.where(dd > 0.0, 1, -1).astype(np.int64)
    tmax = np.stack([boundary(k[:, a], dd[:, a], o[a], h) for a in range(3)], axis=1)
    t_in = np.zeros(len(ray))
    visits = np.ones(len(ray), dtype=np.int64)
    hit = find(k)
    visit_ray, visit_key = [ray.copy()], [k.copy()]
    alive = np.flatnonzero(hit < 0)
    step = 0
    while len(alive):
        tx, ty, tz = tmax[alive, 0], tmax[alive, 1], tmax[alive, 2]
        axis = np.where((tx <= ty) & (tx <= tz), 0, np.where(ty <= tz, 1, 2))
        t_sel = tmax[alive, axis]
        go = (t_sel < te[alive]) & (step < max_steps[alive])
        alive, axis, t_sel = alive[go], axis[go], t_sel[go]
        if not len(alive):
            break
        t_in[alive] = t_sel
        k[alive, axis] += sgn[alive, axis]
        for a in range(3):
            sel = alive[axis == a]
            tmax[sel, a] = boundary(k[sel, a], dd[sel, a], o[a], h)
        visits[alive] += 1
        visit_ray.append(ray[alive])
        visit_key.append(k[alive].copy())
        found = find(k[alive])
        hit[alive] = found
        alive = alive[found < 0]
        step += 1
    # CLASS, in the header's order
    own = e_defined[ray] & np.all(k == ek[ray], axis=1)
    got = hit >= 0
    cls = np.where(~got, OPEN,
                   np.where(own, OWN,
                            np.where(t_in >= 1.0, BEHIND,
                                     np.where(confirmed[np.maximum(hit, 0)] if len(confirmed) else False, CONFIRMED,
                                              np.where(t_in < t_front[ray], BLOCKED, NEAR)))))
    status = np.zeros(n, dtype=np.uint8)
    status[ray] = cls
    rng = np.full(n, np.uint64(NO_HIT_RANGE_BITS)).view(np.float64)
    rng[ray[got]] = (t_in * length[ray])[got]
    hit_key = np.full((n, 3), NO_HIT_KEY, dtype=np.int32)
    hit_key[ray[got]] = k[got].astype(np.int32)
    steps = np.zeros(n, dtype=np.uint32)
    steps[ray] = visits
    hit_all = np.full(n, -1, dtype=np.int64)
    hit_all[ray] = hit
    return Result(status, rng, hit_key, steps, hit_all, np.concatenate(visit_ray), np.concatenate(visit_key))


# ---- the brute force: independent of the order of the rule's operations ---------------------------------------------
def first_hit_brute(map_keys, voxel, pts, T, p: Params, eps_factor=2e-7, chunk=64):
    """The slab method over every (ray, voxel) pair -> (first hit per point: index into map_keys or -1, decided per point,
    casts).  eps = eps_factor * voxel, in metres along the ray.  A ray with a hit is decided when its first box is crossed
    by more than eps, is entered more than eps before t_end, and every other box that the ray may touch (grown by eps) is
    entered more than eps later; a ray without one when no grown box is touched up to t_end + eps."""
    h = float(voxel)
    eps = eps_factor * h
    keys = np.asarray(map_keys, dtype=np.float64).reshape(-1, 3)
    e, o, d, length, t_end, _, casts = rays_of(pts, T, p)
    if not keys_of(o[None, :], h)[1][0]:
        casts[:] = False
    lo, hi = keys * h, keys * h + h
    first = np.full(len(e), -1, dtype=np.int64)
    decided = np.zeros(len(e), dtype=bool)
    ray = np.flatnonzero(casts)
    if len(keys) == 0:
        decided[ray] = True
        return first, decided, casts

    def span(idx, lo_b, hi_b):
        """Entry and exit of every (ray, box), in metres along the ray; entry > exit: not crossed."""
        dd = d[idx][:, None, :] / length[idx][:, None, None]     # unit directions (r, 1, 3)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = (lo_b[None, :, :] - o) / dd
            t2 = (hi_b[None, :, :] - o) / dd
        inside = (o >= lo_b[None, :, :]) & (o <= hi_b[None, :, :])
        flat = dd == 0.0
        near = np.where(flat, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
        far = np.where(flat, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
        return np.maximum(near.max(axis=2), 0.0), far.min(axis=2)

    for at in range(0, len(ray), chunk):
        idx = ray[at:at + chunk]
        end = (t_end[idx] * length[idx])[:, None]
        enter_g, leave_g = span(idx, lo - eps, hi + eps)               # may be touched
        cand = (enter_g <= leave_g) & (enter_g <= end + eps)
        enter_s, leave_s = span(idx, lo + eps, hi - eps)               # certainly crossed
        sure = (leave_s - enter_s > eps) & (enter_s < end - eps)
        entry = np.where(cand, enter_g, np.inf)
        best = np.argmin(entry, axis=1)
        rows = np.arange(len(idx))
        any_cand = cand.any(axis=1)
        others = entry.copy()
        others[rows, best] = np.inf
        clear = others.min(axis=1) > entry[rows, best] + 3.0 * eps     # (grown and shrunk entries differ by up to 2 eps)
        first[idx] = np.where(any_cand, best, -1)
        decided[idx] = np.where(any_cand, sure[rows, best] & clear, True)
    return first, decided, casts


# ---- the scene: a room -----------------------------------------------------------------------------------------------
@dataclass
class Room:
    voxel_size: float
    keys: np.ndarray      # V x 3 int32: the shell, then the stale voxels
    means: np.ndarray     # V x 3: the voxels' centres
    covs: np.ndarray      # V x 9
    stale: np.ndarray     # the stale voxels' keys


def _directions(seed, stream, idx):
    u = np.stack([2.0 * synth.rand_unit(seed, stream + a, idx) - 1.0 for a in range(3)], axis=1)
    u[np.all(u == 0.0, axis=1)] = (1.0, 0.0, 0.0)
    return u / np.sqrt((u * u).sum(axis=1))[:, None]


def make_room(seed=SCENE_SEEDS[0], pose=None):
    """The map: a one-voxel shell at max|k| = SHELL with a window in the +x wall, and STALE voxels 3 - 8 m from the
    sensor (world position of ORIGIN at `pose`)."""
    pose = scene_pose() if pose is None else pose
    r = np.arange(-SHELL, SHELL + 1)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    shell = g[np.abs(g).max(axis=1) == SHELL]
    window = (shell[:, 0] == SHELL) & (np.abs(shell[:, 1]) <= WINDOW) & (np.abs(shell[:, 2]) <= WINDOW)
    shell = shell[~window]
    o = transform(pose, np.asarray(ORIGIN))[0]
    idx = np.arange(2 * STALE, dtype=np.uint64)
    at = o + _directions(seed, 100, idx) * (3.0 + 5.0 * synth.rand_unit(seed, 103, idx))[:, None]
    stale = np.floor(at / VOXEL).astype(np.int64)
    _, keep = np.unique(stale, axis=0, return_index=True)
    stale = stale[np.sort(keep)][:STALE]
    keys = np.concatenate([shell, stale]).astype(np.int32)
    means = (keys.astype(np.float64) + 0.5) * VOXEL
    covs = np.tile((1e-3 * np.eye(3)).reshape(9), (len(keys), 1))
    return Room(VOXEL, keys, np.ascontiguousarray(means), covs, stale.astype(np.int32))


def _wall(o, u):
    """Metres from o along the unit direction u to the shell's inner face, and |u| along that face's normal."""
    inner_hi, inner_lo = SHELL * VOXEL, (-SHELL + 1) * VOXEL
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(u > 0.0, (inner_hi - o) / u, np.where(u < 0.0, (inner_lo - o) / u, np.inf))
    a = np.argmin(s, axis=1)
    rows = np.arange(len(u))
    return s[rows, a], np.abs(u[rows, a])


def make_scene(n, seed=SCENE_SEEDS[0], room=None):
    """A scan of n points (frame of the scan; origin ORIGIN) in the room; the point's kind is i % 8, so that a 63-point
    prefix already holds every kind.  -> (room, points, pose)."""
    pose = scene_pose()
    room = room if room is not None else make_room(seed, pose)
    o = transform(pose, np.asarray(ORIGIN))[0]
    i = np.arange(n, dtype=np.int64)
    idx = i.astype(np.uint64)
    kind = i % 8
    u = _directions(seed, DIRECTION_STREAM, idx)
    f = synth.rand_unit(seed, 303, idx)
    # 4: through the window; 5: through the centre of a stale voxel
    win = np.stack([np.full(n, (SHELL + 0.5) * VOXEL), (2.0 * synth.rand_unit(seed, 304, idx) - 1.0) * (WINDOW * VOXEL),
                    (2.0 * synth.rand_unit(seed, 305, idx) - 1.0) * (WINDOW * VOXEL) + 0.5 * VOXEL], axis=1) - o
    aim = (room.stale[(i // 8) % len(room.stale)].astype(np.float64) + 0.5) * VOXEL - o
    u = np.where((kind == 4)[:, None], win / np.sqrt((win * win).sum(axis=1))[:, None], u)
    u = np.where((kind == 5)[:, None], aim / np.sqrt((aim * aim).sum(axis=1))[:, None], u)
    # 7: the direction of point i - 7 (a point of kind 0)
    back = np.maximum(i - 7, 0)
    u = np.where((kind == 7)[:, None], u[back], u)
    s_wall, normal = _wall(o, u)
    s = np.select([kind <= 2, kind == 3, kind == 4, kind == 5, kind == 6],
                  [s_wall + 0.25, (0.4 + 0.4 * f) * s_wall, 30.0, s_wall + 0.25, s_wall + VOXEL / normal + 0.6],
                  default=s_wall + 0.25 + 0.7)
    world = o + u * s[:, None]
    pts = transform(synth.invert_pose(pose), world)
    return room, np.ascontiguousarray(pts), pose
