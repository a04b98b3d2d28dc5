"""The reference of the map-merge tests (include/vgicp_hip_map_merge.h): the header's rule restated operation by operation
in numpy (float64 ufuncs round every product, sum and quotient once and fuse nothing, which is what the rule asks).  Not a
test module; tests/test_map_merge_cpu.py checks the restatement on its own and pins it against the oracle's insertion,
tests/test_map_merge.py holds the device against it.

THE RULE.  SELECTION and TRANSFORM are the submap's (tests/map_submap_reference.py: too_far, transform); a selected voxel,
moved, is a CONTRIBUTOR (c, m', C').  Its destination voxel is KEY = floor(m'_a / h) per axis, h the destination's voxel
size.  The contributors of one destination voxel are taken in the ORDER they are given in (the device: ascending slot index
of the source table).  FOLD: the state (count, mean, cov) starts as the destination record, or at count 0; for each
contributor
    if max_count != 0 and count >= max_count:  not accepted (frozen += 1)
    elif count == 0:                            mean, cov = m', C' bit for bit; count = c
    else:  nn, cc, n1 = float(count), float(c), float(count + c);  x = (nn * x + cc * x') / n1 for the twelve entries;
           count += c
"""
from dataclasses import dataclass, field

import numpy as np

import map_submap_reference as ms
from map_levels_reference import sort_by_key


def voxel_keys(points, h):
    """The map's key of a point: (int32) floor(x / h) per axis, the quotient rounded once."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.floor(p / np.float64(h)).astype(np.int32)


def fold(count, entries, contributors, max_count=0):
    """One destination voxel.  count: int (0: the voxel does not exist); entries: its twelve doubles (mean, then the
    column-major covariance) or None; contributors: [(c, twelve doubles)] in order.
    -> (count, entries, accepted points, frozen contributors)."""
    count = int(count)
    x = None if entries is None else np.array(entries, dtype=np.float64)
    points = frozen = 0
    for c, y in contributors:
        c, y = int(c), np.asarray(y, dtype=np.float64)
        if max_count != 0 and count >= max_count:
            frozen += 1
            continue
        if count == 0:
            x = y.copy()
            count = c
        else:
            nn, cc, n1 = np.float64(count), np.float64(c), np.float64(count + c)
            x = (nn * x + cc * y) / n1          # three ufuncs and a fourth: each rounds once
            count += c
        points += c
    return count, x, points, frozen


@dataclass
class Merged:
    keys: np.ndarray      # (n, 3) int32, sorted by (x, y, z): the destination map after the call
    means: np.ndarray     # (n, 3)
    covs: np.ndarray      # (n, 9) column-major
    counts: np.ndarray    # (n,) uint64
    created: int = 0
    updated: int = 0
    frozen: int = 0
    points: int = 0
    groups: dict = field(default_factory=dict)   # destination key -> (existed before, number of contributors)

    def export(self):
        return self.keys, self.means, self.covs, self.counts


def merge(dst, points, covs, counts, h, max_count=0):
    """KEY, ORDER and FOLD: the destination's export `dst` = (keys, means, covs, counts), any order, and the moved
    contributors in the order the source's slots give them."""
    dk, dm, dc, dn = (np.asarray(a) for a in dst)
    table = {tuple(int(v) for v in k): [int(n), np.concatenate([m, c]).astype(np.float64)]
             for k, m, c, n in zip(dk.reshape(-1, 3), dm.reshape(-1, 3), dc.reshape(-1, 9), dn.reshape(-1))}
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    covs = np.asarray(covs, dtype=np.float64).reshape(-1, 9)
    counts = np.asarray(counts, dtype=np.uint64).reshape(-1)
    lists, order = {}, []
    for j, key in enumerate(map(tuple, voxel_keys(points, h).tolist())):
        if key not in lists:
            lists[key] = []
            order.append(key)
        lists[key].append((int(counts[j]), np.concatenate([points[j], covs[j]])))
    out = Merged(None, None, None, None)
    for key in order:
        existed = key in table
        count, entries = table[key] if existed else (0, None)
        new_count, new_entries, accepted, frozen = fold(count, entries, lists[key], max_count)
        out.groups[key] = (existed, len(lists[key]))
        out.frozen += frozen
        out.points += accepted
        if accepted:                                  # a voxel that accepted nothing is not written
            table[key] = [new_count, new_entries]
            out.created += 0 if existed else 1
            out.updated += 1 if existed else 0
    keys = np.array(list(table.keys()), dtype=np.int32).reshape(-1, 3)
    payload = np.array([v[1] for v in table.values()], dtype=np.float64).reshape(-1, 12)
    n = np.array([v[0] for v in table.values()], dtype=np.uint64)
    out.keys, out.means, out.covs, out.counts = sort_by_key(keys, payload[:, :3], payload[:, 3:], n)
    return out


def select_and_move(src_in_slot_order, h, center, radius, frame=None, min_count=0):
    """SELECTION and TRANSFORM over the source's voxels GIVEN IN SLOT ORDER: -> (points, covs, counts, (voxels, selected,
    too_far, too_few)), the contributors in that order."""
    keys, means, covs, counts = (np.asarray(a) for a in src_in_slot_order)
    keys, counts = keys.reshape(-1, 3), counts.reshape(-1).astype(np.uint64)
    far = ms.too_far(keys, h, center, radius) if len(keys) else np.zeros(0, dtype=bool)
    enough = np.ones(len(keys), dtype=bool) if min_count <= 1 else counts >= np.uint64(min_count)
    take = ~far & enough
    pts, rot = ms.transform(means.reshape(-1, 3)[take], covs.reshape(-1, 9)[take], np.eye(4) if frame is None else frame)
    return pts, rot, counts[take], (len(keys), int(take.sum()), int(far.sum()), int((~far & ~enough).sum()))


def exports_equal(a, b):
    """Two exports (keys, means, covs, counts), any order: equal by key with == on every double, counts included."""
    a, b = sort_by_key(*a), sort_by_key(*b)
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
