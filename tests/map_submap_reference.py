"""The reference of the submap tests (include/vgicp_hip_map_submap.h): the header's rule restated operation by operation
in numpy (float64 ufuncs round every product and sum once and fuse nothing, which is what the rule asks).  Not a test
module; tests/test_map_submap_cpu.py checks the restatement on hand-worked cases, tests/test_map_submap.py holds the
device against it.

THE RULE.  h is the voxel size of the source table.  A voxel with key K and count c is SELECTED iff
    d_a = ((double)K_a + 0.5) * h - center_a,   !(sqrt((dx dx + dy dy) + dz dz) > radius)      (eviction would keep it)
    and (min_count <= 1 or c >= min_count).
A selected voxel becomes the point ((R[.,0] m0 + R[.,1] m1) + R[.,2] m2) + t with the covariance (R C) R^T, both products
summed left to right.  The device emits the selected voxels in ascending slot order; the content is compared here
sorted by key, which does not depend on where the table put a key.
"""
from dataclasses import dataclass

import numpy as np

from map_levels_reference import sort_by_key


def too_far(keys, h, center, radius):
    """LocalMap::needsPointRemoval per key: True where eviction at `center` with threshold `radius` removes the voxel."""
    k = np.asarray(keys).reshape(-1, 3).astype(np.float64)
    c = np.asarray(center, dtype=np.float64).reshape(3)
    h, radius = np.float64(h), np.float64(radius)
    dx, dy, dz = ((k[:, a] + 0.5) * h - c[a] for a in range(3))
    return np.sqrt((dx * dx + dy * dy) + dz * dz) > radius


def transform(means, covs, frame):
    """(points, covariances) of the voxels under `frame` (4x4): every product and sum rounded once, in the rule's order."""
    m = np.asarray(means, dtype=np.float64).reshape(-1, 3)
    C = np.asarray(covs, dtype=np.float64).reshape(-1, 9)           # column-major: C[r, c] = covs[:, r + 3 c]
    T = np.asarray(frame, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    pts = np.stack([((R[r, 0] * m[:, 0] + R[r, 1] * m[:, 1]) + R[r, 2] * m[:, 2]) + t[r] for r in range(3)], axis=1)
    RC = {(r, c): (R[r, 0] * C[:, 3 * c] + R[r, 1] * C[:, 1 + 3 * c]) + R[r, 2] * C[:, 2 + 3 * c] for r in range(3) for c in range(3)}
    out = np.zeros_like(C)
    for c in range(3):
        for r in range(3):
            out[:, r + 3 * c] = (RC[r, 0] * R[c, 0] + RC[r, 1] * R[c, 1]) + RC[r, 2] * R[c, 2]
    return pts.reshape(-1, 3), out


@dataclass
class Submap:
    keys: np.ndarray      # (n, 3) int32, sorted by (x, y, z)
    points: np.ndarray    # (n, 3)
    covs: np.ndarray      # (n, 9) column-major
    counts: np.ndarray    # (n,) uint64
    voxels: int           # the four counts of vgicp_submap_stats
    too_far: int
    too_few: int

    def __len__(self):
        return len(self.keys)


def submap(keys, means, covs, counts, h, center, radius, frame=None, min_count=0):
    """The rule over a whole table, given as the arrays an export returns (any order)."""
    keys = np.asarray(keys, dtype=np.int32).reshape(-1, 3)
    means = np.asarray(means, dtype=np.float64).reshape(-1, 3)
    covs = np.asarray(covs, dtype=np.float64).reshape(-1, 9)
    counts = np.asarray(counts, dtype=np.uint64).reshape(-1)
    far = too_far(keys, h, center, radius)
    enough = np.ones(len(keys), dtype=bool) if min_count <= 1 else counts >= np.uint64(min_count)
    take = ~far & enough
    pts, rot = transform(means[take], covs[take], np.eye(4) if frame is None else frame)
    k, p, c, n = sort_by_key(keys[take], pts, rot, counts[take])
    return Submap(k, p, c, n, len(keys), int(far.sum()), int((~far & ~enough).sum()))


def by_key(keys, points, covs, counts):
    """What the device delivered (scan order), sorted by key like Submap."""
    return sort_by_key(np.asarray(keys, dtype=np.int32).reshape(-1, 3), np.asarray(points).reshape(-1, 3),
                       np.asarray(covs).reshape(-1, 9), np.asarray(counts, dtype=np.uint64).reshape(-1))


# ---- the purpose, end to end: a piece of one map registered on another --------------------------------------------------
VOXEL = 0.5
CAP = 20
FRAMES = 6
RADIUS = 15.0
MIN_COUNT = 2
ALIGN = dict(max_iteration=100, translation_sq_threshold=1e-6, cosine_threshold=0.9999)


def offset():
    """D: 2 degrees about z and 0.2 m, inside one voxel of VOXEL."""
    a = np.deg2rad(2.0)
    D = np.eye(4)
    D[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    D[:3, 3] = (0.15, -0.12, 0.05)
    return D


def two_sessions(oracle):
    """One scene, two maps from disjoint frame sets of synth.make_sensor_stream.  -> (frames A, frames B, D, anchor): a
    list of (points, covs, pose) per map, A from the even frames at their true poses, B from the odd frames at
    D^-1 * true pose, so that D takes B's map onto A's; the anchor is the pose of B's first frame in B's map."""
    from eskf_lio_amd import synth
    events, truth = synth.make_sensor_stream(frames=FRAMES, points_per_frame=6000)
    sweeps = [e[1] for _, e in events if e[0] == "lidar"]
    D = offset()
    Dinv = synth.invert_pose(D)
    a, b = [], []
    for k, sweep in enumerate(sweeps):
        p, c, _ = oracle.preprocess(sweep, VOXEL, 30)
        (a if k % 2 == 0 else b).append((p, c, truth[k][1] if k % 2 == 0 else Dinv @ truth[k][1]))
    return a, b, D, Dinv @ truth[1][1]


def anchor_error(pose, D, anchor):
    """Metres between the anchor's pose in A's map as registered and as D puts it."""
    return float(np.linalg.norm(np.asarray(pose)[:3, 3] - (D @ anchor)[:3, 3]))
