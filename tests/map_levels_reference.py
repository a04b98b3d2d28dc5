"""The reference of the map-level tests (include/vgicp_hip_map_levels.h): the header's rule restated operation by operation
in numpy (float64 ufuncs round every product, sum and quotient once and fuse nothing, which is what the rule asks), and
the recipe of the coarse-to-fine experiment both test files run.  Not a test module; tests/test_map_levels_cpu.py checks
the restatement on its own, tests/test_map_levels.py holds the device against it.

THE RULE.  Level 0 is the map.  Level l >= 1 has voxel size voxel_size * 2^l and is derived from level l-1 alone:
  * a level-l voxel exists for every key K = k >> 1 (arithmetic shift per component) of a voxel k of level l-1;
  * its children are the up to eight voxels 2K + (dx, dy, dz) of level l-1, taken in octant order o = dx + 2 dy + 4 dz;
  * with ONE child, mean, covariance and count are the child's, bit for bit;
  * with more, N = sum of count_c (integers), and every entry of mean and covariance is
        (sum over the children in octant order of (double)count_c * entry_c) / (double)N
    where the sum starts from the first child's product and every product, sum and quotient is rounded once;
  * count = N.
"""
from dataclasses import dataclass

import numpy as np

from eskf_lio_amd import synth

LEVELS_MAX = 4            # VGICP_LEVELS_MAX
LEVEL_STAGES_MAX = 8      # VGICP_LEVEL_STAGES_MAX


@dataclass
class Level:
    keys: np.ndarray      # (n, 3) int32, sorted by (x, y, z)
    means: np.ndarray     # (n, 3)
    covs: np.ndarray      # (n, 9) column-major
    counts: np.ndarray    # (n,) uint64

    def __len__(self):
        return len(self.keys)


def sort_by_key(keys, *arrays):
    """keys (n, 3) and the arrays that go with them, in ascending (x, y, z) order."""
    keys = np.asarray(keys).reshape(-1, 3)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return (keys[order],) + tuple(np.asarray(a)[order] for a in arrays)


def as_level(keys, means, covs, counts):
    k, m, c, n = sort_by_key(np.asarray(keys, dtype=np.int32).reshape(-1, 3), np.asarray(means, dtype=np.float64).reshape(-1, 3),
                             np.asarray(covs, dtype=np.float64).reshape(-1, 9), np.asarray(counts, dtype=np.uint64).reshape(-1))
    return Level(k, m, c, n)


def coarsen(fine: Level) -> Level:
    """One step of the rule: level l from level l-1."""
    n = len(fine)
    if n == 0:
        return Level(np.zeros((0, 3), np.int32), np.zeros((0, 3)), np.zeros((0, 9)), np.zeros(0, np.uint64))
    k = fine.keys.astype(np.int64)
    parent = k >> 1                                             # arithmetic: -1 -> -1
    octant = (k[:, 0] & 1) + 2 * (k[:, 1] & 1) + 4 * (k[:, 2] & 1)
    pkeys, index = np.unique(parent, axis=0, return_inverse=True)   # ascending (x, y, z)
    index = index.reshape(-1)
    m = len(pkeys)
    payload = np.concatenate([fine.means, fine.covs], axis=1)   # the twelve entries go the same way
    present = np.zeros((m, 8), dtype=bool)
    child = np.zeros((m, 8), dtype=np.int64)
    present[index, octant] = True
    child[index, octant] = np.arange(n)
    total = np.zeros(m, dtype=np.uint64)
    acc = np.zeros((m, 12))
    started = np.zeros(m, dtype=bool)
    for o in range(8):                                          # octant order
        has = present[:, o]
        c = child[:, o]
        cnt = np.where(has, fine.counts[c], np.uint64(0)).astype(np.uint64)
        total = total + cnt                                     # integers
        prod = cnt.astype(np.float64)[:, None] * payload[c]     # rounded once
        first = has & ~started
        acc[first] = prod[first]                                # the sum STARTS from the first child's product
        later = has & started
        acc[later] = acc[later] + prod[later]                   # rounded once
        started |= has
    out = acc / total.astype(np.float64)[:, None]               # rounded once
    single = present.sum(axis=1) == 1
    only = child[np.arange(m), np.argmax(present, axis=1)]
    out[single] = payload[only[single]]                         # one child: its bits
    return Level(pkeys.astype(np.int32), out[:, :3].copy(), out[:, 3:].copy(), total)


def levels_of(keys, means, covs, counts, levels):
    """[level 0 (the map itself, sorted), level 1, ..., level `levels`]."""
    out = [as_level(keys, means, covs, counts)]
    for _ in range(levels):
        out.append(coarsen(out[-1]))
    return out


def same_level(a: Level, b: Level):
    """Bit for bit: keys, means, covariances and counts (both sorted by key)."""
    return (a.keys.shape == b.keys.shape and np.array_equal(a.keys, b.keys) and np.array_equal(a.counts, b.counts)
            and a.means.tobytes() == b.means.tobytes() and a.covs.tobytes() == b.covs.tobytes())


# ---- the coarse-to-fine experiment ------------------------------------------------------------------------------------
VOXEL = 0.3
CAP = 1000
SCAN_POINTS = 6000
SCHEDULE = (3, 2, 1, 0)
COARSE = dict(max_iteration=30, translation_sq_threshold=1e-4, cosine_threshold=0.999)
FINE = dict(max_iteration=100, translation_sq_threshold=1e-6, cosine_threshold=0.9999)
SHIFTS = (0.3, 0.6, 0.9, 1.2)             # metres along x: the guesses the plain align fails from
FAR_LIMIT = VOXEL / 2                     # "the plain align sits in another voxel"
NEAR_LIMIT = VOXEL / 30                   # "the chain ends where the plain align from the identity ends"


def recipe(oracle, map_points=20000, scan_points=SCAN_POINTS):
    """-> (map points, map covs, scan points, scan covs): the scene at seed 1 prepared at 0.3 m / 30 neighbours is the
    map, the first `scan_points` kept points of the same scene at seed 2 are the scan."""
    mp, mc, _ = oracle.preprocess(synth.make_lidar_scan(map_points, seed=1), VOXEL, 30)
    sp, sc, _ = oracle.preprocess(synth.make_lidar_scan(map_points, seed=2), VOXEL, 30)
    return mp, mc, sp[:scan_points], sc[:scan_points]


def shifted(dx):
    T = np.eye(4)
    T[0, 3] = dx
    return T


def distance(a, b):
    return float(np.linalg.norm(np.asarray(a)[:3, 3] - np.asarray(b)[:3, 3]))


def oracle_level_map(oracle, level: Level, voxel_size):
    """An OracleMap of the level's size that holds the level: every voxel's (mean, cov) inserted as one point."""
    omap = oracle.OracleMap(voxel_size, 1)
    omap.insert(level.means, level.covs)
    return omap


def oracle_chain(oracle, level_maps, sp, sc, guess, schedule=SCHEDULE, coarse=COARSE, fine=FINE):
    """The schedule on the oracle: stage i against level schedule[i], the last with `fine`, from the previous pose.
    -> (pose, [OracleAlign per stage])."""
    pose, stages = np.asarray(guess, dtype=np.float64), []
    for i, l in enumerate(schedule):
        p = fine if i == len(schedule) - 1 else coarse
        r = level_maps[l].align(sp, sc, pose, p["max_iteration"], p["translation_sq_threshold"], p["cosine_threshold"])
        stages.append(r)
        pose = r.pose
    return pose, stages
