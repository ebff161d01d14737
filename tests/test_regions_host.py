"""tests/regions_ref.py, the reference of the region grid, checked without a device: its labels against scipy.ndimage.label
and, on small shapes, against an all-pairs reachability closure; its records against a scene whose result can be derived
by hand; and the package's structures against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import regions_ref as R
from tests import regions_scenes as RS
from tests.conftest import ROOT

SHAPES = [(1, 1), (1, 70), (70, 1), (32, 32), (33, 31), (64, 32), (65, 33), (128, 64), (129, 65)]
RANGES = [(0, 98), (100, 100), (-1, -1)]


def canonical(lab):
    """scipy's labels 1 .. n as the least linear index of each component, NONE for 0"""
    out = np.full(lab.shape, R.NONE, np.uint32)
    flat, of = lab.ravel(), out.ravel()
    first = {}
    for i, v in enumerate(flat):
        if v:
            first.setdefault(int(v), i)
            of[i] = first[int(v)]
    return out


def scipy_labels(m, conn4):
    structure = ndimage.generate_binary_structure(2, 1) if conn4 else np.ones((3, 3), int)
    return canonical(ndimage.label(m, structure=structure)[0])


def planes_of(w, h):
    rng = np.random.default_rng(1000 * w + h)
    return {"random": S.random_plane(rng, w, h), "serpentine": S.serpentine(w, h), "spiral": S.spiral(w, h),
            "diagonal_gaps": S.diagonal_gaps(w, h), "pocket": S.pocket(w, h), "full": RS.full(w, h), "empty": RS.empty(w, h),
            "dots": RS.dots(w, h), "staircase": RS.staircase(w, h), "frontier": RS.frontier_plane(w, h)}


@pytest.mark.parametrize("w,h", SHAPES)
def test_labels_against_scipy(w, h):
    for name, plane in planes_of(w, h).items():
        for lo, hi in RANGES:
            m = R.members(plane, R.params(R.BYTES, lo, hi))
            for conn4 in (False, True):
                assert np.array_equal(R.label(m, conn4), scipy_labels(m, conn4)), (name, lo, hi, conn4)
        for flags in (0, R.NEIGHBOURS_8, R.EDGE_UNKNOWN, R.NEIGHBOURS_8 | R.EDGE_UNKNOWN):
            m = R.members(plane, R.params(R.FRONTIER, flags=flags))
            for conn4 in (False, True):
                assert np.array_equal(R.label(m, conn4), scipy_labels(m, conn4)), (name, flags, conn4)


def test_the_scenes_do_what_they_are_for():
    w, h = 129, 65
    by = R.params(R.BYTES, 100, 100)
    assert R.extract(RS.full(w, h), by)["summary"] == dict(cells_member=w * h, regions=1, regions_recorded=1, regions_listed=1,
                                                           largest_cells=w * h)
    assert R.extract(RS.empty(w, h), by)["summary"] == dict.fromkeys(R.SUMMARY_KEYS, 0)
    for flags in (0, R.CONNECT_4):
        s = R.extract(RS.dots(w, h), R.params(R.BYTES, 100, 100, flags=flags), max_regions=3)["summary"]
        assert s["regions"] == 65 * 33 and s["regions_recorded"] == 3 and s["largest_cells"] == 1
    assert R.extract(RS.staircase(w, h), by)["summary"]["regions"] == 1
    assert R.extract(RS.staircase(w, h), R.params(R.BYTES, 100, 100, flags=R.CONNECT_4))["summary"]["regions"] == 65
    free = R.params(R.BYTES, 0, 98)
    assert R.extract(S.serpentine(w, h), free)["summary"]["largest_cells"] == 4289
    assert R.extract(S.spiral(w, h), free)["summary"]["largest_cells"] == 4290
    # the frontier plane: the counts the issue gives
    for (fw, fh), regions, cells in (((32, 32), 10, 415), ((65, 33), 30, 872), ((129, 65), 64, 3496)):
        s = R.extract(RS.frontier_plane(fw, fh), R.params(R.FRONTIER))["summary"]
        print((fw, fh), s)
        assert s["regions"] > 1 and s["cells_member"] > 100


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (5, 4), (9, 7), (7, 9)])
def test_labels_against_the_reachability_closure(w, h):
    rng = np.random.default_rng(w * 31 + h)
    n = w * h
    for trial in range(12):
        m = rng.random((h, w)) < (0.35, 0.5, 0.65)[trial % 3]
        for conn4 in (False, True):
            reach = np.eye(n, dtype=bool)
            for y in range(h):
                for x in range(w):
                    for dx, dy in (R.EDGE_STEPS if conn4 else R.ALL_STEPS):
                        nx, ny = x + dx, y + dy
                        if 0 <= nx < w and 0 <= ny < h and m[y, x] and m[ny, nx]:
                            reach[y * w + x, ny * w + nx] = True
            for _ in range(7):                                       # 2^7 >= 63 steps
                reach = (reach.astype(np.uint8) @ reach.astype(np.uint8)) > 0
            want = np.array([int(np.argmax(reach[i])) if m.ravel()[i] else R.NONE for i in range(n)], np.uint32).reshape(h, w)
            assert np.array_equal(R.label(m, conn4), want), (trial, conn4)


def test_a_room_with_two_doors():
    """FREE inside OCCUPIED walls inside UNKNOWN, a door gap of 5 cells in the west wall and one of 2 cells in the east wall:
    exactly two frontier regions, the gaps; the robot stands near the east door"""
    plane, west, east = RS.room()
    h, w = plane.shape
    geo = N.geometry(0.25, 0.0, 0.0, w, h)
    robot = (w - 9, 18)
    cost = np.where(plane == 0, 0, 100).astype(np.int8)
    field = N.solve(geo, cost, N.params(50, 3, 400, 98), np.array([robot], np.int32))
    assert field["summary"]["goals_used"] == 1
    P = field["P"]
    for rank, first in ((R.RANK_CELLS, west), (R.RANK_POTENTIAL, east), (R.RANK_LABEL, west)):
        got = R.extract(plane, R.params(R.FRONTIER, rank=rank), cost, P)
        assert not got["error"]
        assert got["summary"] == dict(cells_member=7, regions=2, regions_recorded=2, regions_listed=2, largest_cells=5)
        lst = got["list"]
        cells_of = [{(int(x), int(y)) for y, x in np.argwhere(got["labels"] == r["label"])} for r in lst]
        assert cells_of[0] == first and cells_of[1] == ({*west, *east} - first)
        for r, cells in zip(lst, cells_of):
            assert (int(r["centre_x"]), int(r["centre_y"])) in cells and (int(r["entry_x"]), int(r["entry_y"])) in cells
            assert int(r["entry_potential"]) == min(int(P[y, x]) for x, y in cells)
            assert int(r["label"]) == min(y * w + x for x, y in cells)
        assert [tuple(g) for g in R.goals(lst, R.GOAL_CENTRE)] == [(int(r["centre_x"]), int(r["centre_y"])) for r in lst]
    west_record = R.extract(plane, R.params(R.FRONTIER, rank=R.RANK_CELLS), cost, P)["list"][0]
    assert (west_record["centre_x"], west_record["centre_y"]) == (5, 12) and west_record["cells"] == 5
    assert (west_record["min_x"], west_record["min_y"], west_record["max_x"], west_record["max_y"]) == (5, 10, 5, 14)
    assert (west_record["sum_x"], west_record["sum_y"]) == (25, 60)
    # min_cells drops the narrow door; without a potential the entry is the centre
    alone = R.extract(plane, R.params(R.FRONTIER, min_cells=3))
    assert alone["summary"]["regions_listed"] == 1 and alone["summary"]["regions_recorded"] == 2
    r = alone["list"][0]
    assert (r["entry_x"], r["entry_y"], r["entry_potential"]) == (r["centre_x"], r["centre_y"], R.UNREACHED)
    # a rank by potential needs one
    assert R.extract(plane, R.params(R.FRONTIER, rank=R.RANK_POTENTIAL))["error"]


def test_centroid_rounding_and_ties():
    assert [R.centroid(s, 2) for s in (0, 1, 2, 3)] == [0, 1, 1, 2]      # a half rounds up
    assert R.centroid(7, 3) == 2 and R.centroid(4, 3) == 1 and R.centroid(8191 * 5, 5) == 8191
    # two cells side by side: the centroid cell is the right one, which is then the centre; a 2 x 2 block ties four ways
    # around (1, 1), itself a member: distance 0 wins
    plane = np.zeros((4, 6), np.int8)
    plane[0, 0:2] = 100
    plane[2:4, 3:5] = 100
    got = R.extract(plane, R.params(R.BYTES, 100, 100))
    a, b = got["records"]
    assert (a["centroid_x"], a["centroid_y"], a["centre_x"], a["centre_y"]) == (1, 0, 1, 0)
    assert (b["centroid_x"], b["centroid_y"], b["centre_x"], b["centre_y"]) == (4, 3, 4, 3)
    # a ring: the centroid cell is no member, four members tie, the least index wins
    ring = np.zeros((5, 5), np.int8)
    ring[1:4, 1:4] = 100
    ring[2, 2] = 0
    r = R.extract(ring, R.params(R.BYTES, 100, 100, flags=R.CONNECT_4))["records"][0]
    assert (r["centroid_x"], r["centroid_y"], r["centre_x"], r["centre_y"], r["cells"]) == (2, 2, 2, 1, 8)


def test_structures_and_symbols(lom):
    hdr = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in re.findall(r"\b(lom_regions_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)):
        assert name in lom.capi.EXPORTED, name
    assert C.sizeof(lom.capi.RegionsParams) == 20 and lom.capi.REGIONS_RECORD.itemsize == 48
    assert lom.capi.REGIONS_RECORD == R.RECORD
    for name, value in (("NONE", R.NONE), ("BYTES", R.BYTES), ("FRONTIER", R.FRONTIER), ("NEIGHBOURS_8", R.NEIGHBOURS_8),
                        ("EDGE_UNKNOWN", R.EDGE_UNKNOWN), ("CONNECT_4", R.CONNECT_4), ("RANK_LABEL", R.RANK_LABEL),
                        ("RANK_CELLS", R.RANK_CELLS), ("RANK_POTENTIAL", R.RANK_POTENTIAL), ("GOAL_CENTRE", R.GOAL_CENTRE),
                        ("GOAL_ENTRY", R.GOAL_ENTRY)):
        assert getattr(lom.capi, "REGIONS_" + name) == value
        assert re.search(r"LOM_REGIONS_%s\s*=?\s*(0x[0-9A-Fa-f]+u?|\d+)" % name, hdr), name
    p = lom.regionsParams(R.as_tuple(R.params(R.FRONTIER, -3, 7, 50, 4, R.RANK_CELLS, 5)))
    assert (p.kind, p.lo, p.hi, p.max_cost, p.min_cells, p.rank, p.flags) == (1, -3, 7, 50, 4, 1, 5)
    assert hasattr(lom, "RegionGrid")
