"""The reference of the locate tests (include/vgicp_hip_map_locate.h): the header's rule restated operation by operation in
numpy (float64 ufuncs round every product, sum and quotient once and fuse nothing, which is what the rule asks), a brute
force of it, and the recipe of the experiment both test files run.  Not a test module; tests/test_map_locate_cpu.py
checks the restatement on its own, tests/test_map_locate.py holds the device against it.

THE RULE.  h = voxel_size * 2^level.  Only points with i % stride == 0 take part.  e = T p by the insertion's transform,
((R[.,0] x0 + R[.,1] x1) + R[.,2] x2) + t per row; K = floor(e / h) per axis, defined iff all three are within +-2^30; a
point whose key is not defined (e not finite included) is skipped and counted.  A cell is a shift d with |d_a| <= w_a; its
index is c = ((dz + wz)(2 wy + 1) + (dy + wy))(2 wx + 1) + (dx + wx).  hits[c] = the points that take part and are not
skipped for which the level holds a voxel with the key K + d.  The best cell is the LOWEST index that attains the
maximum; its pose is the input pose with t_a + (double)d_a * h added per axis.
"""
from dataclasses import dataclass

import numpy as np

import map_levels_reference as ml

MAX_POSES = 64            # VGICP_LOCATE_MAX_POSES
MAX_HALF_WIDTH = 32       # VGICP_LOCATE_MAX_HALF_WIDTH
MAX_CELLS = 4096          # VGICP_LOCATE_MAX_CELLS
KEY_LIMIT = 2.0 ** 30


def transform(T, pts):
    """e = T p, the insertion's transform: left to right, every product and sum rounded once."""
    T = np.asarray(T, dtype=np.float64)
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)


def keys_of(e, h):
    """-> (keys int64 (n, 3), defined bool (n,)): floor(e / h) per axis, defined iff all three are within +-2^30."""
    with np.errstate(all="ignore"):
        q = np.floor(e / h)
        defined = np.all(np.abs(q) <= KEY_LIMIT, axis=1)          # NaN compares false
    return np.where(defined[:, None], q, 0.0).astype(np.int64), defined


def cells_of(window):
    """-> (cells, 3) int64: the shifts d in the order of the cell index (dx fastest, dz slowest)."""
    wx, wy, wz = (int(v) for v in window)
    dz, dy, dx = np.meshgrid(np.arange(-wz, wz + 1), np.arange(-wy, wy + 1), np.arange(-wx, wx + 1), indexing="ij")
    return np.stack([dx.reshape(-1), dy.reshape(-1), dz.reshape(-1)], axis=1).astype(np.int64)


class KeySet:
    """The keys of a level's voxels, for exact membership queries of many keys at once.  A key's components are ranked
    among the level's own values per axis (a value the level does not have is a miss), and the rank triple is one int64."""

    def __init__(self, keys):
        k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
        self.axes = [np.unique(k[:, a]) for a in range(3)]
        self.packed = np.unique(self._pack(*[np.searchsorted(self.axes[a], k[:, a]) for a in range(3)]))

    def _pack(self, ix, iy, iz):
        return (ix * max(len(self.axes[1]), 1) + iy) * max(len(self.axes[2]), 1) + iz

    def contains(self, q):
        q = np.asarray(q, dtype=np.int64).reshape(-1, 3)
        if len(self.packed) == 0:
            return np.zeros(len(q), dtype=bool)
        ok, idx = np.ones(len(q), dtype=bool), []
        for a in range(3):
            i = np.minimum(np.searchsorted(self.axes[a], q[:, a]), len(self.axes[a]) - 1)
            ok &= self.axes[a][i] == q[:, a]
            idx.append(i)
        p = self._pack(*idx)
        j = np.minimum(np.searchsorted(self.packed, p), len(self.packed) - 1)
        return ok & (self.packed[j] == p)


@dataclass
class Best:
    hits: int
    cell: int
    offset: tuple
    points: int
    skipped: int
    pose: np.ndarray          # 4 x 4

    def as_dict(self):
        return dict(hits=self.hits, cell=self.cell, offset=self.offset, points=self.points, skipped=self.skipped)


def score(keyset: KeySet, h, pts, T, window, stride=1, cell_block=256):
    """One pose -> (hits uint32 (cells,), points, skipped).  Equal keys are grouped first and counted with their
    multiplicity, which changes no number."""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)[::int(stride)]
    K, defined = keys_of(transform(T, p), h)
    uniq, mult = np.unique(K[defined], axis=0, return_counts=True)
    d = cells_of(window)
    hits = np.zeros(len(d), dtype=np.uint32)
    if len(uniq):
        for c0 in range(0, len(d), cell_block):
            q = uniq[None, :, :] + d[c0:c0 + cell_block, None, :]
            found = keyset.contains(q.reshape(-1, 3)).reshape(len(q), len(uniq))
            hits[c0:c0 + cell_block] = (found * mult[None, :]).sum(axis=1)
    return hits, int(defined.sum()), int((~defined).sum())


def best_of(hits, window, T, h, points, skipped):
    c = int(np.argmax(hits))          # the first maximum: the lowest index
    d = cells_of(window)[c]
    pose = np.array(T, dtype=np.float64)
    for a in range(3):
        pose[a, 3] = pose[a, 3] + float(d[a]) * h          # one product, one sum
    return Best(int(hits[c]), c, tuple(int(v) for v in d), points, skipped, pose)


def locate(level_keys, h, pts, poses, window, stride=1):
    """-> ([Best per pose], hits uint32 (k, cells)) of the rule, for a level given by its keys and voxel size."""
    keyset = level_keys if isinstance(level_keys, KeySet) else KeySet(level_keys)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    bests, planes = [], []
    for T in poses:
        hits, points, skipped = score(keyset, h, pts, T, window, stride)
        planes.append(hits)
        bests.append(best_of(hits, window, T, h, points, skipped))
    return bests, np.stack(planes)


def brute_force(level_keys, h, pts, T, window, stride=1):
    """The plain triple loop over (point, cell, voxel), in Python integers: hits (cells,)."""
    voxels = [tuple(int(v) for v in k) for k in np.asarray(level_keys).reshape(-1, 3)]
    K, defined = keys_of(transform(T, np.asarray(pts, dtype=np.float64).reshape(-1, 3)), h)
    d = cells_of(window)
    hits = np.zeros(len(d), dtype=np.uint32)
    for i in range(len(K)):
        if i % stride != 0 or not defined[i]:
            continue
        for c in range(len(d)):
            want = (int(K[i, 0] + d[c, 0]), int(K[i, 1] + d[c, 1]), int(K[i, 2] + d[c, 2]))
            for v in voxels:
                if v == want:
                    hits[c] += 1
    return hits


# ---- the experiment ----------------------------------------------------------------------------------------------------
LEVEL = 3
WINDOW = (4, 4, 1)
YAWS = 64
KEEP = 4
STRIDES = (1, 4)
# (translation in metres, yaw in degrees) of the wrong guess [Rz(yaw) | t]; the first three are the cases for which the
# chain from the wrong guess itself is run too
WRONG_GUESSES = (((5.1, -3.7, 0.5), 37.0), ((-7.3, 6.2, -0.4), -110.0), ((2.0, 1.0, 0.0), 180.0),
                 ((8.5, 8.5, 0.9), 2.8125), ((-8.0, 3.0, -0.9), 92.8125), ((0.0, 0.0, 0.0), 47.8125))
CHAIN_CASES = 3


def rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def wrong_guess(translation, yaw_degrees):
    T = np.eye(4)
    T[:3, :3] = rot_z(np.deg2rad(yaw_degrees))
    T[:3, 3] = translation
    return T


def yaw_fan(guess, count):
    """Pose j is [Rz(2 pi j / count) R_guess | t_guess]: a rotation about the world's z through the sensor's position."""
    guess = np.asarray(guess, dtype=np.float64)
    out = np.tile(guess, (count, 1, 1))
    for j in range(count):
        out[j, :3, :3] = rot_z(2.0 * np.pi * j / count) @ guess[:3, :3]
    return out


def ranking(bests):
    """Pose indices by best hits, descending, ties to the lower index."""
    hits = np.array([b.hits if isinstance(b, Best) else b["hits"] for b in bests], dtype=np.int64)
    return [int(i) for i in np.argsort(-hits, kind="stable")]


@dataclass
class Candidate:
    index: int            # of the pose in the fan
    hits: int
    offset: tuple
    start: np.ndarray     # the located pose, where the chain starts
    pose: np.ndarray      # where the chain ends
    rounds: list          # per stage
    matches: int          # level-0 matches at `pose`


def matches_at(keyset0, pts, pose):
    """Scan points that fall into a voxel of the map at `pose`: locate's own count with a window of one cell."""
    return int(score(keyset0, ml.VOXEL, pts, pose, (0, 0, 0))[0][0])


def pipeline(oracle, level_maps, keysets, sp, sc, guess, level=LEVEL, window=WINDOW, stride=1, yaws=YAWS, keep=KEEP):
    """Locate on the yaw fan about `guess`, the oracle's chain from the `keep` best poses, the winner by level-0 matches
    (ties to the earlier candidate).  keysets[l]: the KeySet of level l.  -> (winner, [Candidate])."""
    fan = yaw_fan(guess, yaws)
    bests, _ = locate(keysets[level], ml.VOXEL * 2 ** level, sp, fan, window, stride)
    out = []
    for j in ranking(bests)[:keep]:
        pose, stages = ml.oracle_chain(oracle, level_maps, sp, sc, bests[j].pose)
        out.append(Candidate(j, bests[j].hits, bests[j].offset, bests[j].pose, pose, [s.iterations for s in stages],
                             matches_at(keysets[0], sp, pose)))
    winner = max(out, key=lambda c: c.matches)          # max() keeps the first of equals
    return winner, out
