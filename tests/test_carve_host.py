"""Ray carving, the parts that need no GPU: the reference walk (tests/carve_ref.py) visits exactly the cells the
segment meets -- checked against geometry, independently of any kernel --, the C ABI is declared, and bad arguments
are refused before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import carve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_map_carve_rays", "lom_map_carve_rays_device", "lom_map_carve_counts", "lom_odometry_set_carve",
               "lom_odometry_get_carve_stats"]


def _generic_rays(seed, voxel, origin_cell, n):
    """Random rays with no coordinate on a plane: origin inside the given cell (0 = the double-width one), endpoints
    1.5 .. 18 voxels away in every direction."""
    rng = np.random.default_rng(seed)
    V = float(np.float32(voxel))
    oc = np.asarray(origin_cell, np.float64)
    lo, hi = R.cell_bounds(oc, V)
    origin = (lo + (hi - lo) * rng.uniform(0.1, 0.9, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = (origin + d * rng.uniform(1.5 * V, 18 * V, (n, 1))).astype(np.float32)
    return origin, pts


@pytest.mark.parametrize("voxel", [0.2, 0.5])
@pytest.mark.parametrize("origin_cell", [(3, 2, 1), (-2, -4, -1), (0, 0, 0), (0, -1, 2)])
def test_walk_visits_exactly_the_cells_the_segment_meets(voxel, origin_cell):
    p = R.params(margin=0.3 * voxel, min_range=voxel, max_range=15 * voxel, min_crossings=1)
    seed = 100 * int(voxel * 10) + 10 * abs(origin_cell[0]) + abs(origin_cell[1])  # one per case
    origin, pts = _generic_rays(seed, voxel, origin_cell, 120)
    V = float(np.float32(voxel))
    w = R.walk(origin, pts, voxel, p)
    assert not w["error"]
    t_end, walked, _ = R.t_end_of(origin, pts, p)
    assert walked.all() and (t_end < 1).all()
    assert (np.sort(np.unique(w["ray"])) == np.arange(len(pts))).all()
    O = origin.astype(np.float64)
    assert tuple(R.map_index(origin[None], voxel)[0][0]) == tuple(origin_cell)
    clipped = 0
    for i in range(len(pts)):
        D = pts[i].astype(np.float64) - O
        got = [tuple(c) for c in w["cell"][w["ray"] == i].tolist()]
        assert len(set(got)) == len(got), i                                   # a cell at most once
        assert got[0] == tuple(origin_cell), i
        steps = np.abs(np.diff(np.array(got), axis=0)).sum(1) if len(got) > 1 else np.zeros(0)
        assert (steps == 1).all(), i                                          # one face at a time
        want = R.cells_met_by_segment(O, D, float(t_end[i]), V)
        assert set(got) == want, (i, sorted(set(got) ^ want))
        clipped += np.linalg.norm(D) > p["max_range"]
    assert clipped > 0 and clipped < len(pts)  # both forms of t_end occur


def test_plane_rule_and_cell_zero():
    """cell 0 is (-V, V): a ray along +x from x = -0.75 (V = 0.5) visits -1, 0, 1 and never a second cell 0"""
    p = R.params(margin=0.0, min_range=0.1, max_range=10.0, min_crossings=1)
    w = R.walk([-0.75, 0.1, 0.1], [[0.75, 0.1, 0.1]], 0.5, p)
    assert w["cell"][:, 0].tolist() == [-1, 0, 1] and not w["cell"][:, 1:].any()
    w = R.walk([0.75, 0.1, 0.1], [[-0.75, 0.1, 0.1]], 0.5, p)
    assert w["cell"][:, 0].tolist() == [1, 0, -1]
    # lattice diagonal, three-way ties: x, then y, then z
    w = R.walk([0.25, 0.25, 0.25], [[1.25, 1.25, 1.25]], 0.5, p)
    assert w["cell"].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 1, 1], [2, 2, 1], [2, 2, 2]]


def test_reference_range_errors_and_skips():
    p = R.params(margin=0.5, min_range=1.0, max_range=5.0, min_crossings=1)
    assert R.walk([0, 0, 0], [[np.nan, 0, 0]], 0.5, p)["error"]
    assert R.walk([0, 0, 0], [[0.5 * 2.0 ** 20, 0, 0]], 0.5, p)["error"]
    assert R.walk([np.inf, 0, 0], [[1, 0, 0]], 0.5, p)["error"]
    w = R.walk([0.1, 0.1, 0.1], [[0.1, 0.1, 0.1], [0.6, 0.1, 0.1], [0.1, 1.35, 0.1], [0.1, 0.1, 9.0]], 0.5,
               dict(p, margin=1.5))
    assert w["walked"].tolist() == [False, False, False, True]  # L == 0, L < min_range, L <= margin, L > max_range


def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"#define\s+LOM_ABI_VERSION\s+2\b", text)
    assert lom.capi.lib().lom_abi_version() == 2
    assert re.search(r"ray carving", text, re.I)
    assert C.sizeof(lom.capi.CarveParams) == 16 and C.sizeof(lom.capi.CarveStats) == 40
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    assert re.search(r"\bcarveRays\s*\(", mirror) and re.search(r"\bsetCarve\s*\(", mirror)


def test_bad_arguments_are_refused(lom):
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    good = lom.carveParams(R.params(0.3, 1.0, 60.0, 2))
    o3 = (C.c_float * 3)(0, 0, 0)
    xyz = np.zeros((4, 3), np.float32)
    st = lom.capi.CarveStats()
    for fn in (L.lom_map_carve_rays, L.lom_map_carve_rays_device):
        assert fn(None, o3, xyz.ctypes.data, 4, 12, C.byref(good), C.byref(st)) == ERR_ARG
        assert fn(None, o3, xyz.ctypes.data, 0, 12, C.byref(good), None) == ERR_ARG
    assert L.lom_map_carve_counts(None, o3, xyz.ctypes.data, 4, 12, C.byref(good), None, None, 0) == ERR_ARG
    assert L.lom_odometry_set_carve(None, C.byref(good)) == ERR_ARG
    assert L.lom_odometry_set_carve(None, None) == ERR_ARG
    assert L.lom_odometry_get_carve_stats(None, C.byref(st)) == ERR_ARG
    bad = [dict(margin=-0.1), dict(margin=float("nan")), dict(margin=float("inf")), dict(min_range=0.0),
           dict(min_range=-1.0), dict(min_range=float("nan")), dict(max_range=1.0), dict(max_range=0.5),
           dict(max_range=float("nan")), dict(max_range=float("inf")), dict(min_crossings=0)]
    for change in bad:
        p = lom.carveParams(dict(R.params(0.3, 1.0, 60.0, 2), **change))
        assert L.lom_odometry_set_carve(None, C.byref(p)) == ERR_ARG, change
        assert L.lom_map_carve_rays(None, o3, xyz.ctypes.data, 4, 12, C.byref(p), None) == ERR_ARG, change
    with pytest.raises(TypeError):
        lom.carveParams(dict(margin=0.3))  # no defaults: all four fields or none
