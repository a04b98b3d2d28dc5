"""What the constructions of tests/knn_paths_reference.py promise, as far as geometry decides it, without a device: the
cell counts that make the kernel open, measure or spill, the tied band's width and ties in the kernel's own expression,
the grid edge's cell indices, the start lists' classification — and that the oracle accepts every scan.  Whether the
device then takes the path is asserted by tests/test_knn_paths.py from the search report; here also the report's
header against its Python mirror and the libraries' exports."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import knn_paths_reference as kp
from eskf_lio_amd import capi
from test_evaluate_cpu import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header, mirror, libraries -----------------------------------------------------------------------------------------
def test_header_declares_the_one_function_and_the_library_exports_it():
    lib = capi.load_library()
    assert declared("vgicp_hip_search_report.h") == sorted(capi.SEARCH_REPORT_EXPORTS) == ["vgicp_prepare_search_report"]
    text = open(os.path.join(ROOT, "include", "vgicp_hip_search_report.h")).read()
    assert '#include "vgicp_hip.h"' in text and "libvgicp_hip_search_report.so" in text
    assert not re.search(r"#define\s+VGICP_OPTION_", text)
    body = re.search(r"typedef struct vgicp_search_report \{(.*?)\} vgicp_search_report;", text, re.S).group(1)
    fields = re.findall(r"^\s*uint32_t (\w+);", body, re.M)
    assert fields == [name for name, _ in capi.SearchReport._fields_] and len(fields) == 24
    assert tuple(fields[10:]) == capi.SEARCH_PATHS == kp.PATHS
    import ctypes as C
    assert C.sizeof(capi.SearchReport) == 96
    out = subprocess.run(["nm", "-D", "--defined-only", capi.side_lib_path("search_report")], capture_output=True, text=True,
                         check=True).stdout
    assert set(re.findall(r" T (vgicp_[a-z_0-9]+)", out)) == set(capi.SEARCH_REPORT_EXPORTS)
    assert hasattr(lib, "vgicp_prepare_search_report")


def test_module_exports_stay_as_they_are_and_the_kernels_bits_follow_the_struct():
    lib = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgicp_[a-z_0-9]+)", out))
    assert not set(capi.SEARCH_REPORT_EXPORTS) & exported and lib.vgicp_abi_version() == 6
    assert "search_report" not in open(os.path.join(ROOT, "include", "vgicp_hip.h")).read()
    # the kernel's bits (vgicp_device.h) in the order of the struct's fields
    text = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "vgicp_device.h")).read()
    bits = {name: int(bit) for name, bit in re.findall(r"constexpr uint32_t kPath(\w+) = 1u << (\d+);", text)}
    camel = ["".join(part.capitalize() for part in name.split("_")) for name in kp.PATHS]
    assert [bits[name] for name in camel] == list(range(14)) and len(bits) == 14
    assert re.search(r"constexpr int kPathWord0 = 81;", text) and re.search(r"constexpr int kPathCount = 14;", text)
    # the constants the constructions are sized by
    src = open(os.path.join(ROOT, "eskf_lio_amd", "csrc", "vgicp_preprocess.hip")).read()
    for name, value in (("kFineShift", kp.FINE_SHIFT), ("kLevels", kp.LEVELS), ("kPool", kp.POOL),
                        ("kLeafPoints", kp.LEAF_POINTS), ("kHomePoints", kp.HOME_POINTS), ("kHeavyLevel", kp.HEAVY_LEVEL),
                        ("kHeavyBelow", kp.HEAVY_BELOW), ("kKnnSelectLow", kp.SELECT_LOW)):
        assert re.search(r"constexpr \w+ %s = %d;" % (name, value), src), name


# ---- the constructions ---------------------------------------------------------------------------------------------------
def test_shell():
    """Fewer than 30 points closer than the shell (one: the centre), so the 30th distance is the shell's; the centre's
    cells below level 6 hold only itself and its level-6 cell more than 128 points (crowded); all eight octant cells
    hold more than 1 024 points (opened, two levels down); their level-4 children together exceed the pool."""
    scan = kp.shell()
    assert len(scan) == 12_001
    d = np.sqrt(kp.kernel_d2(scan, kp.SHELL_CENTRE))
    assert (d < kp.SHELL_RADIUS * (1 - 1e-3)).sum() == 1 < kp.KNN and d[1:].max() < kp.SHELL_RADIUS * (1 + 1e-3)
    own = kp.own_cell_counts(scan, scan[0])
    assert own[:6] == [1] * 6 and own[6] > kp.HOME_POINTS
    octants = kp.cell_counts(scan, 6)
    assert len(octants) == 8 and min(octants.values()) > kp.LEAF_POINTS
    children = collections.Counter(tuple(v >> 2 for v in key) for key in kp.cell_counts(scan, 4))
    counts = sorted(children.values())
    # seven octants' children and the eighth octant's cell fit the pool, the eighth's children do not
    assert sum(counts) > kp.POOL >= sum(counts[1:]) + 1 and max(kp.cell_counts(scan, 4).values()) <= kp.LEAF_POINTS
    assert list(kp.kept_indices(scan)[:1]) == [0]


def test_blob():
    scan = kp.blob()
    cells = kp.cell_counts(scan, 1)
    assert cells == {(0, 0, 0): 1, (1, 0, 0): 1_200} and cells[1, 0, 0] > kp.LEAF_POINTS
    assert list(kp.kept_indices(scan)) == [0]                     # the query is the scan's one kept point
    own = kp.own_cell_counts(scan, scan[0])
    assert own[:2] == [1, 1] and own[2] > kp.HOME_POINTS              # no home: crowded at the voxel level
    assert max(kp.cell_counts(scan, 0).values()) < kp.LEAF_POINTS


@pytest.mark.parametrize("cfg", [kp.BAND_HOME, kp.BAND_FAR], ids=["home", "far"])
def test_tied_band(cfg):
    """In the kernel's expression: 20 points within 0.02 m; at least 96 points whose squared distances lie within 2^-10
    relative of one another and in one bucket of the select's 16-bit key; 48 exact ties among them; 25 points closer
    than the ties, so the 30th neighbour is a tie and five ties are chosen by index."""
    scan, info = kp.tied_band(**cfg)
    d2 = kp.kernel_d2(scan, info["query"])
    kind = info["kind"]
    assert d2[0] == 0.0 and kind[0] == -1 and (kind == 0).sum() == 20 and np.sqrt(d2[kind == 0].max()) < 0.02
    band = d2[kind >= 1]
    assert len(band) >= 96 and (band.max() - band.min()) / band.min() < 2.0 ** -10
    assert len(set(kp.select_bucket(band))) == 1
    assert (d2 == info["tie_d2"]).sum() == (kind == 1).sum() == 48
    assert (d2 < info["tie_d2"]).sum() == 21 + kp.BAND_BELOW < kp.KNN
    order = np.lexsort((np.arange(len(scan)), d2))[:kp.KNN]
    ties = np.flatnonzero(kind == 1)
    assert set(order[kind[order] == 1]) == set(ties[:5]) and ties[4] > ties[:4].max() > 5   # index order, not geometry
    assert not np.array_equal(np.argsort(d2[1:], kind="stable"), np.arange(len(scan) - 1))
    own = kp.own_cell_counts(scan, scan[0])
    if cfg is kp.BAND_HOME:
        assert own[0] < kp.KNN <= own[1] == len(scan) <= kp.HOME_POINTS      # home: the level-1 cell holds the whole scan
    else:
        assert max(own) < kp.KNN and len(kp.cell_counts(scan, 4)) == 8      # no own cell; the band lies across 8 level-4 cells
    assert kp.kept_indices(scan)[0] == 0


def test_far_clusters_pile_and_exactly_k():
    far = kp.far_clusters()
    assert len(far) == 45 and max(max(kp.own_cell_counts(far, p)) for p in far) < kp.KNN
    pile = kp.pile()
    dup = np.all(pile == kp.PILE_POINT, axis=1)
    assert dup.sum() == 700 and max(kp.cell_counts(pile, 0).values()) >= 700 > kp.HOME_POINTS and len(pile) == 1_040
    assert len(kp.exactly(30)) == kp.KNN and len(kp.exactly(17)) == 17 < kp.KNN


def test_grid_edge(oracle):
    scan = kp.grid_edge()
    c = kp.fine_cells(scan, kp.EDGE_VOXEL)
    assert c.min() == -kp.COORD_OFFSET and c.max() == kp.COORD_OFFSET - 1
    assert set(np.unique(c[:40])) == set(kp.EDGE_LOW) and set(np.unique(c[40:80])) == set(kp.EDGE_HIGH)
    for lo, cells in ((80, kp.EDGE_LOW), (160, kp.EDGE_HIGH)):
        block = c[lo:lo + 80]
        assert set(np.unique(block[:, [0, 2]])) == set(cells) and set(np.unique(block[:, 1])) == {-2, -1, 0, 1}
        assert (block[:, 1] < 0).sum() == 40 and list(block[:2, 1]) == [-1, 0]
        for q in (lo, lo + 1):
            # a query whose own cells stop at y = 0 on every level, with some of its 30 nearest beyond that face
            own = kp.own_cell_counts(scan, scan[q], kp.EDGE_VOXEL)
            assert own[0] < kp.KNN <= own[1] == max(own) == 40
            nearest = np.argsort(kp.kernel_d2(scan, scan[q]), kind="stable")[:kp.KNN]
            other = (c[nearest, 1] < 0) != (c[q, 1] < 0)
            assert 1 <= other.sum() < kp.KNN and np.all((nearest >= lo) & (nearest < lo + 80))
    assert list(c[0]) == [kp.EDGE_LOW[0]] * 3 and list(c[40]) == [kp.EDGE_HIGH[1]] * 3
    # the map's own floor agrees on the voxels: the outermost voxel index at either end, +-2^17
    v = oracle.voxel_index(kp.EDGE_VOXEL, scan)
    assert np.array_equal(v, c >> kp.FINE_SHIFT) and v.min() == -(1 << 17) and v.max() == (1 << 17) - 1
    kept = kp.kept_indices(scan, kp.EDGE_VOXEL)
    assert kept[0] == 0 and {40, 80, 81, 160, 161} <= set(kept)   # the edge cells' points are queries
    for q in (0, 40):
        own = kp.own_cell_counts(scan, scan[q], kp.EDGE_VOXEL)
        assert own[0] < kp.KNN <= own[1] == 40
    beyond = kp.fine_cells(kp.one_cell_beyond(scan), kp.EDGE_VOXEL)
    assert beyond.max() == kp.COORD_OFFSET and (beyond >= kp.COORD_OFFSET).sum() == 1


def test_start_lists():
    """Every point a voxel of its own; the classification by a numpy count of level-4 cells; the sizes for which no light
    block exists are exactly 1, 7 and 17."""
    for n in kp.START_SIZES:
        scan = kp.all_heavy(n)
        assert len(kp.kept_indices(scan)) == n and kp.heavy_light(scan) == (n, 0)
        assert max(kp.cell_counts(scan, kp.HEAVY_LEVEL).values()) == 1
    assert kp.LIGHT_SIZES == (8, 9, 15, 16, 63, 64, 65)
    for n in kp.LIGHT_SIZES:
        scan = kp.all_light(n)
        assert len(scan) == len(kp.kept_indices(scan)) == n and kp.heavy_light(scan) == (0, n)
        assert min(kp.cell_counts(scan, kp.HEAVY_LEVEL).values()) >= kp.HEAVY_BELOW
    from test_knn_paths import MIXED
    assert {a % 8 for a, _ in MIXED} == {0, 1, 7} and {b for _, b in MIXED} == set(kp.MIXED_HEAVY)
    for n_light, n_heavy in MIXED:
        scan = kp.mixed(n_light, n_heavy)
        assert len(kp.kept_indices(scan)) == n_light + n_heavy and kp.heavy_light(scan) == (n_heavy, n_light)


def test_the_oracle_accepts_every_scan_and_decoys_cover_them(oracle):
    """oracle.preprocess runs on every construction and keeps what the numpy count keeps; the decoy of every scan keeps
    at least as many points (it writes every output slot the scan's preparation writes) and shares no point with it."""
    from test_knn_paths import CONSTRUCTIONS, MIXED
    scans = [(make(), voxel, knn) for make, voxel, knn, _ in CONSTRUCTIONS.values()]
    scans += [(kp.all_heavy(n), kp.VOXEL, kp.KNN) for n in kp.START_SIZES]
    scans += [(kp.all_light(n), kp.VOXEL, kp.KNN) for n in kp.LIGHT_SIZES]
    scans += [(kp.mixed(a, b), kp.VOXEL, kp.KNN) for a, b in MIXED]
    for scan, voxel, knn in scans:
        rp, rc, ri = oracle.preprocess(scan, voxel, knn)
        assert np.array_equal(ri.astype(np.int64), kp.kept_indices(scan, voxel)) and np.isfinite(rc).all()
        d = kp.decoy(len(scan), 0, voxel)
        assert len(kp.kept_indices(d, voxel)) >= len(ri) and d.shape == scan.shape
        assert not set(map(tuple, d)) & set(map(tuple, scan))
