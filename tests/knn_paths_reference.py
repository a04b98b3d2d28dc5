"""Scans built so that the neighbour search of the scan preparation (knn_search_kernel, eskf_lio_amd/csrc/
vgicp_preprocess.hip) takes one named path each, and the geometry of that kernel restated in numpy so that the CPU tests
can check what the constructions promise.  tests/test_knn_paths_cpu.py checks the geometry, tests/test_knn_paths.py runs
the scans on the device against the oracle and asserts, from Context.search_report(), that the path was taken.

Only the kept points of a scan (the first input index of every voxel) are queries; a construction around one query
therefore puts that query FIRST in its voxel.  Every scan here stands alone (nothing else within 20 m)."""
import itertools

import numpy as np

VOXEL, KNN = 0.3, 30
# the kernel's constants (vgicp_preprocess.hip)
FINE_SHIFT, LEVELS, COORD_OFFSET = 2, 12, 1 << 19
LEAF_POINTS, HOME_POINTS, POOL = 1024, 128, 256
HEAVY_LEVEL, HEAVY_BELOW = 4, 4
SELECT_LOW = 15                      # the select resolves bits 30..15 of the single-precision key
PATHS = ("home", "crowded", "no_own_cell", "window_is_k", "whole_scan", "clipped", "open2", "open1", "leaf", "finest",
         "compacted", "spilled", "waited", "reranked")


# ---- the kernel's geometry -------------------------------------------------------------------------------------------
def fine_cells(points, voxel=VOXEL):
    """floor(p / fine) per axis, the kernel's finest cell index before its offset (cell_coord without the clamp)."""
    fine = voxel / (1 << FINE_SHIFT)
    return np.floor(np.asarray(points, dtype=np.float64) / fine).astype(np.int64)


def cell_counts(points, level, voxel=VOXEL):
    """{cell index at `level` (3-tuple): points in it}."""
    keys, counts = np.unique(fine_cells(points, voxel) >> level, axis=0, return_counts=True)
    return {tuple(int(v) for v in k): int(c) for k, c in zip(keys, counts)}


def own_cell_counts(points, query, voxel=VOXEL):
    """Points in the query's own cell on every level 0..LEVELS-1."""
    c, q = fine_cells(points, voxel), fine_cells(query, voxel)
    return [int(np.all((c >> l) == (q >> l), axis=1).sum()) for l in range(LEVELS)]


def kept_indices(points, voxel=VOXEL):
    """First input index of every voxel, ascending: the queries of the search."""
    keys = np.floor(np.asarray(points, dtype=np.float64) / voxel).astype(np.int64)
    _, first = np.unique(keys, axis=0, return_index=True)
    return np.sort(first)


def heavy_light(points, voxel=VOXEL):
    """(n_heavy, n_light) as query_split_body sorts the kept points: heavy = the own level-4 cell holds fewer than 4
    points of the scan (all points, kept or not)."""
    c4 = fine_cells(points, voxel) >> HEAVY_LEVEL
    keys, inverse, counts = np.unique(c4, axis=0, return_inverse=True, return_counts=True)
    per_point = counts[np.asarray(inverse).reshape(-1)]
    kept = kept_indices(points, voxel)
    heavy = int((per_point[kept] < HEAVY_BELOW).sum())
    return heavy, len(kept) - heavy


def kernel_d2(points, query):
    """The kernel's expression dx*dx + dy*dy + dz*dz, in float64, operation by operation."""
    d = np.asarray(points, dtype=np.float64) - np.asarray(query, dtype=np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def select_bucket(d2):
    """The 16 leading bits (below the sign) of the select's key: the distance in single precision, rounded up."""
    d2 = np.asarray(d2, dtype=np.float64)
    f = d2.astype(np.float32)
    f = np.where(f.astype(np.float64) < d2, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)
    return f.view(np.uint32) >> SELECT_LOW


def decoy(n, seed, voxel=VOXEL):
    """n points that share nothing with any scan here, each in a voxel of its own (so that the decoy keeps n points and
    its preparation writes every output slot): a random choice of every second voxel of a cube beside (5, 5, 5) m,
    a random place inside the voxel."""
    rng = np.random.default_rng(1_000_003 + seed)
    side = int(np.ceil(max(n, 1) ** (1.0 / 3.0))) + 1
    cells = rng.permutation(side ** 3)[:n]
    cells = np.stack([cells % side, (cells // side) % side, cells // (side * side)], axis=1)
    return 5.0 + voxel * (2.0 * cells + rng.uniform(0.1, 0.9, size=(n, 3)))


# ---- a. shell: spilled, compacted, open2, leaf, crowded ------------------------------------------------------------
SHELL_CENTRE = np.array([0.01, 0.02, 0.03])
SHELL_RADIUS = 4.7


def shell(n=12_000, seed=1):
    """One centre point and n points on the sphere of radius 4.7 m around it (relative radial jitter 1e-4).  The
    centre's own level-6 cell (4.8 m) is the positive octant; each octant cell holds n / 8 > 1 024 points, so it is
    opened two levels down, and the children of the first seven fill the pool of 256.  Index 0 is the centre."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    pts = SHELL_CENTRE + v * SHELL_RADIUS * (1.0 + 1e-4 * rng.normal(size=(n, 1)))
    return np.concatenate([SHELL_CENTRE[None], pts])


# ---- b. blob beside a lonely query: open1 ----------------------------------------------------------------------------
BLOB_QUERY = np.array([0.07, 0.07, 0.07])
BLOB_LO, BLOB_HI = np.array([0.16, 0.01, 0.01]), np.array([0.29, 0.14, 0.14])


def blob(n=1_200, seed=2):
    """The query (index 0: the kept point of the one voxel) and n points uniform in the level-1 cell beside its own:
    more than 1 024 in one 0.15 m cell, which is opened one level down."""
    rng = np.random.default_rng(seed)
    return np.concatenate([BLOB_QUERY[None], rng.uniform(BLOB_LO, BLOB_HI, size=(n, 3))])


# ---- c. tied band: reranked, waited, ties by index -------------------------------------------------------------------
TIE_OFFSET, NEAR_TIE_OFFSET = (1, 6, 8), (2, 4, 9)        # 1 + 36 + 64 = 4 + 16 + 81 = 101
BAND_BELOW = 4                                            # near ties just inside the tie radius; the others just outside
BAND_HOME = dict(query=9.0 / 128.0, unit=3.0 / 512.0, near_ties=48)       # radius 0.0589 m inside the cell [0, 0.15)^3
BAND_FAR = dict(query=1.0 / 1024.0, unit=13.0 / 128.0, near_ties=96)      # radius 1.0207 m around a corner of every level


def _orbit(offset):
    """All sign changes and permutations of one offset with three distinct non-zero entries: 48 points."""
    out = {tuple(s * v for s, v in zip(signs, perm))
           for perm in itertools.permutations(offset) for signs in itertools.product((-1, 1), repeat=3)}
    return np.array(sorted(out), dtype=np.float64)


def tied_band(query, unit, near_ties, seed=3):
    """(scan, info).  Index 0: the query (query, query, query), dyadic.  Then, in an order permuted with `seed`: 20
    points within 0.02 m; 48 exact ties at squared distance 101 unit^2 (the orbit of (1, 6, 8) unit: every coordinate
    and every difference is exact in binary, and so is the sum of squares in any order); `near_ties` points on the
    orbit of (2, 4, 9) unit scaled by 1 + e, |e| <= 2^-13, BAND_BELOW of them inside and the rest outside.  The k = 30
    nearest are the query, the 20, the BAND_BELOW and the 5 exact ties of lowest index."""
    rng = np.random.default_rng(seed)
    q = np.full(3, float(query))
    v = rng.normal(size=(20, 3))
    near = q + v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.002, 0.018, size=(20, 1))
    ties = q + _orbit(TIE_OFFSET) * unit
    orbit = _orbit(NEAR_TIE_OFFSET)
    orbit = orbit[np.arange(near_ties) % len(orbit)]
    e = rng.uniform(2.0 ** -15, 2.0 ** -13, size=(near_ties, 1))
    e[:BAND_BELOW] *= -1.0
    near_tie = q + orbit * unit * (1.0 + e)
    rest = np.concatenate([near, ties, near_tie])
    kind = np.concatenate([np.zeros(20, int), np.ones(len(ties), int), np.full(near_ties, 2)])
    perm = rng.permutation(len(rest))
    scan = np.concatenate([q[None], rest[perm]])
    return scan, dict(query=q, tie_d2=101.0 * unit * unit, kind=np.concatenate([[-1], kind[perm]]))


# ---- d. far clusters: whole_scan, no_own_cell ------------------------------------------------------------------------
def far_clusters(seed=3):
    """20, 20 and 5 points at 0, +900 m and -400 m (the clusters of test_preprocess_edge_cases): no cell holds 30 points
    and no level's block covers a ball that reaches the next cluster."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(size=(20, 3)) * 0.05, rng.normal(size=(20, 3)) * 0.05 + 900.0,
                           rng.normal(size=(5, 3)) * 0.05 - 400.0])


# ---- e. pile: crowded at level 0, finest -----------------------------------------------------------------------------
PILE_POINT = np.array([0.51, -0.23, 0.07])


def pile(seed=17):
    """700 duplicates of one point, 300 points around them, 40 duplicates apart (the pile of
    test_preprocess_ties_duplicates_and_crowded_cells), permuted."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([np.tile(PILE_POINT[None], (700, 1)), rng.normal(size=(300, 3)) * 0.4,
                          np.tile([[3.0, 3.0, 3.0]], (40, 1))])
    return pts[rng.permutation(len(pts))]


# ---- f. exactly K: window_is_k ---------------------------------------------------------------------------------------
def exactly(n, seed=5):
    """n points a few metres apart: with n <= knn the opening window holds exactly K = n entries."""
    return np.random.default_rng(seed + n).normal(size=(n, 3)) * 3.0


# ---- g. grid edge: clipped -------------------------------------------------------------------------------------------
EDGE_VOXEL = 0.01
EDGE_LOW, EDGE_HIGH = (-524288, -524287), (524286, 524287)      # the two outermost finest cells at either end


def grid_edge(seed=7):
    """Voxel size 0.01 (finest cells of 0.0025 m, the grid's edge at +-1 310.72 m).
      [0, 40)    40 points in the 2 x 2 x 2 outermost finest cells of the grid's lowest corner (coordinate (c + 0.5) fine
                 plus an offset that stays inside cell c; index 0: the outermost cell itself);
      [40, 80)   40 in those of its highest corner (index 40: the outermost cell);
      [80, 160)  at the low edge in x and z, 40 points either side of y = 0 (cells -2, -1 / 0, 1): two voxels, whose
                 kept points (80: cell -1, 81: cell 0) have their own cells on one side of y = 0 on every level and
                 neighbours on the other side, in cells of the 27-cell block that lie AT the edge;
      [160, 240) the same at the high edge in x and z (160: cell -1, 161: cell 0);
      [240, 440) 200 ordinary points around the origin."""
    rng = np.random.default_rng(seed)
    fine = EDGE_VOXEL / (1 << FINE_SHIFT)

    def place(idx):
        return (idx + 0.5) * fine + rng.uniform(-0.3, 0.3, size=idx.shape) * fine

    def corner(cells, first):
        c = rng.integers(0, 2, size=(40, 3))
        c[0] = first
        return place(np.asarray(cells)[c])

    def face(cells):
        idx = np.asarray(cells)[rng.integers(0, 2, size=(80, 3))]
        idx[:, 1] = np.where(np.arange(80) % 2 == 0, -1, 0) - rng.integers(0, 2, size=80) * np.where(np.arange(80) % 2 == 0, 1, -1)
        idx[0, 1], idx[1, 1] = -1, 0
        return place(idx)
    return np.concatenate([corner(EDGE_LOW, 0), corner(EDGE_HIGH, 1), face(EDGE_LOW), face(EDGE_HIGH),
                           rng.normal(size=(200, 3)) * 0.02])


def one_cell_beyond(scan):
    """The scan with one coordinate moved to the first cell past the grid's upper edge: refused."""
    out = scan.copy()
    out[41, 1] = (524288 + 0.5) * (EDGE_VOXEL / (1 << FINE_SHIFT))
    return out


# ---- start lists ---------------------------------------------------------------------------------------------------
START_SIZES = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)
LATTICE = 0.31
LONELY_FROM, LONELY_STEP = 40.0, 2.0
MIXED_HEAVY = (1, 7, 9)


def all_heavy(n, first=0.05):
    """n points 2 m apart on a line: every level-4 cell (1.2 m) holds one point."""
    x = first + LONELY_STEP * np.arange(n)
    return np.stack([x, np.full(n, 0.05), np.full(n, 0.05)], axis=1)


def all_light(n):
    """A block of the 0.31 m lattice with n points, each in a voxel of its own, such that every level-4 cell it touches
    holds at least 4 of them; None when no block does.  The block is nx x ny x nz lattice points starting at lattice
    index (sx, sy, sz) (0.31 m steps from 0.01 m): the first in lexicographic order of (nz, ny, nx, sz, sy, sx)."""
    for nz, ny in itertools.product(range(1, n + 1), repeat=2):
        if n % (nz * ny) or nz > ny:
            continue
        nx = n // (nz * ny)
        if ny > nx:
            continue
        for sz, sy, sx in itertools.product(range(4), repeat=3):
            ax = [0.01 + LATTICE * (s + np.arange(k)) for s, k in ((sx, nx), (sy, ny), (sz, nz))]
            pts = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
            if min(cell_counts(pts, HEAVY_LEVEL).values()) >= HEAVY_BELOW and len(kept_indices(pts)) == n:
                return pts
    return None


LIGHT_SIZES = tuple(n for n in START_SIZES if all_light(n) is not None)


def mixed(n_light, n_heavy, seed=11):
    """The light block of n_light points and n_heavy lonely points from 40 m on, in an order permuted with `seed`."""
    pts = np.concatenate([all_light(n_light), all_heavy(n_heavy, first=LONELY_FROM)])
    return pts[np.random.default_rng(seed + n_light + n_heavy).permutation(len(pts))]
