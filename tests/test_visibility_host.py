"""The visibility grid without a GPU: the reference (tests/visibility_ref.py) against an independent walk on fractions, its
two forms against each other, the seen set on a free plane, hand cases, the selection's properties, the library's
direction table against numpy's, and the structures and symbols of the ABI."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import navfield_scenes as S
from tests import visibility_ref as V
from tests.conftest import ROOT


def library_table(lom, beams):
    return lom.visibilityTable(beams)


# ---- the walk ------------------------------------------------------------------------------------------------------------------
def fraction_walk(plane, x0, y0, dx, dy, p):
    """An independent walk: the ray leaves the centre of the start cell along (dx, dy); its k-th crossing of a cell border
    along an axis with |d| > 0 lies at the parameter t = (2 k - 1) / (2 |d|).  The crossings are taken in the order of t
    as exact fractions; two at the same t are a corner.  Returns (cells marked, d2, reason)."""
    h, w = plane.shape
    R, block_min, D = p["range_cells"], p["block_min"], p["unknown_depth"]
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    kx = ky = 1                                                       # the next crossing along each axis
    x, y, unknown, cells = x0, y0, 0, []

    def blocking(cx, cy):
        return 0 <= cx < w and 0 <= cy < h and plane[cy, cx] >= block_min

    while True:
        tx = Fraction(2 * kx - 1, 2 * abs(dx)) if dx else None
        ty = Fraction(2 * ky - 1, 2 * abs(dy)) if dy else None
        both = tx is not None and ty is not None and tx == ty
        x_first = ty is None or (tx is not None and tx < ty)
        here = (kx - 1) ** 2 + (ky - 1) ** 2
        if both and blocking(x + sx, y) and blocking(x, y + sy):
            return cells, here, V.END_CORNER
        nx, ny = (x + sx if both or x_first else x), (y + sy if both or not x_first else y)
        nkx, nky = (kx + 1 if both or x_first else kx), (ky + 1 if both or not x_first else ky)
        if not (0 <= nx < w and 0 <= ny < h):
            return cells, here, V.END_EDGE
        if (nkx - 1) ** 2 + (nky - 1) ** 2 > R * R:
            return cells, here, V.END_RANGE
        x, y, kx, ky = nx, ny, nkx, nky
        cells.append((x, y))
        if plane[y, x] >= block_min:
            return cells, (kx - 1) ** 2 + (ky - 1) ** 2, V.END_HIT
        if plane[y, x] < 0:
            unknown += 1
            if D and unknown == D:
                return cells, (kx - 1) ** 2 + (ky - 1) ** 2, V.END_UNKNOWN


@pytest.mark.parametrize("w,h", [(13, 9), (9, 13), (1, 7), (4, 1), (1, 1)])
def test_reference_walk_equals_the_walk_on_fractions(lom, w, h):
    table = library_table(lom, 64)
    rng = np.random.default_rng(100 * w + h)
    ends = set()
    for trial, (block_min, depth) in enumerate(((100, 0), (50, 1), (100, 2))):
        plane = S.random_plane(rng, w, h, obstacles=0.15, unknown=0.2 + 0.1 * trial)
        p = V.params(64, 6, block_min, depth)
        rows = plane.tolist()
        for y0 in range(h):
            for x0 in range(w):
                for b in range(64):
                    dx, dy = int(table[b, 0]), int(table[b, 1])
                    got, want = V.walk(rows, x0, y0, dx, dy, p), fraction_walk(plane, x0, y0, dx, dy, p)
                    assert got == want, (x0, y0, b, got, want)
                    ends.add(got[2])
    if w * h > 50:
        assert ends == {V.END_EDGE, V.END_RANGE, V.END_HIT, V.END_UNKNOWN, V.END_CORNER}


def same_cast(a, b):
    return (a["summary"] == b["summary"] and a["records"].tobytes() == b["records"].tobytes() and a["beams"].tobytes() == b["beams"].tobytes()
            and a["windows"].tobytes() == b["windows"].tobytes() and a["sets"] == b["sets"])


def test_the_two_forms_of_the_reference_agree(lom):
    rng = np.random.default_rng(5)
    for w, h, beams, rng_cells, block_min, depth in ((13, 9, 64, 6, 100, 0), (33, 17, 360, 20, 50, 1), (20, 20, 8, 40, 100, 5), (7, 5, 4, 0, 100, 0)):
        plane = S.random_plane(rng, w, h, obstacles=0.1, unknown=0.3)
        vp = np.array([[0, 0], [w - 1, h - 1], [w // 2, h // 2], [w // 2, h // 2], [-1, 0], [0, h], [w, 2]] +
                      [[int(rng.integers(0, w)), int(rng.integers(0, h))] for _ in range(6)], np.int32)
        p = V.params(beams, rng_cells, block_min, depth)
        slow, fast = V.cast(plane, vp, library_table(lom, beams), p), V.cast_fast(plane, vp, library_table(lom, beams), p)
        assert same_cast(slow, fast)
        r = slow["records"]
        assert (r["unknown"] + r["free"] + r["blocked"] == r["seen"]).all() and (r["valid"][4:7] == 0).all()
        assert (slow["beams"][4:7] == 0).all() and (slow["windows"][4:7] == 0).all() and (r["seen"][r["valid"] == 1] >= 1).all()
        assert slow["records"][2].tobytes() == slow["records"][3].tobytes()       # duplicates are cast independently
    assert V.cast(plane, vp, None, V.params(3, 5))["error"] and V.cast_fast(plane, vp, None, V.params(64, 255))["error"]
    assert V.cast(plane, vp, None, V.params(64, 5, 101))["error"] and V.cast(plane, vp, None, V.params(64, 5, flags=4))["error"]


@pytest.mark.parametrize("R,B,cells", [(5, 64, 81), (10, 64, 317), (20, 128, 1257), (40, 256, 5025)])
def test_free_plane_seen_set_is_the_disc(lom, R, B, cells):
    side = 2 * R + 1
    got = V.cast(np.zeros((side, side), np.int8), [[R, R]], library_table(lom, B), V.params(B, R))
    yy, xx = np.mgrid[0:side, 0:side]
    disc = (xx - R) ** 2 + (yy - R) ** 2 <= R * R
    assert int(disc.sum()) == cells
    r = got["records"][0]
    assert (r["seen"], r["free"], r["unknown"], r["blocked"], r["hits"]) == (cells, cells, 0, 0, 0)
    why, d2 = got["beams"][0] >> 24, got["beams"][0] & 0xFFFFFF
    assert np.isin(why, (V.END_RANGE, V.END_EDGE)).all() and (why[::B // 4] == V.END_EDGE).all() and (d2 <= R * R).all()
    # ... and a subset of the disc for a B that leaves gaps
    few = V.cast_fast(np.zeros((side, side), np.int8), [[R, R]], library_table(lom, 8), V.params(8, R))
    assert 0 < few["records"][0]["seen"] < cells


# ---- hand cases ----------------------------------------------------------------------------------------------------------------
def test_a_diagonal_passes_a_corner_unless_both_side_cells_block(lom):
    table = library_table(lom, 8)
    assert table[1].tolist() == [23170, 23170]                        # beam 1 runs exactly through the cell corners
    p = V.params(8, 10, flags=V.KEEP_BEAMS)
    plane = np.zeros((5, 5), np.int8)
    plane[1, 2] = plane[2, 1] = 100                                   # (2, 1) and (1, 2): the side cells of the step (1, 1) -> (2, 2)
    closed = V.cast(plane, [[1, 1]], table, p)
    assert closed["beams"][0, 1] == (V.END_CORNER << 24) | 0
    assert closed["records"][0]["seen"] == 1 + 2 + 5                   # the start, the two side cells by beams 0 and 2, five free ones
    plane[2, 1] = 0
    gap = V.cast(plane, [[1, 1]], table, p)
    assert gap["beams"][0, 1] == (V.END_EDGE << 24) | 18              # on to (4, 4): three steps each way
    cells = V.walk(plane.tolist(), 1, 1, 23170, 23170, p)[0]
    assert cells == [(2, 2), (3, 3), (4, 4)]                          # the side cells are never marked by this beam
    # a side cell outside the grid does not block
    edge = np.zeros((3, 3), np.int8)
    edge[1, 0] = 100
    assert V.walk(edge.tolist(), 0, 0, -23170, 23170, p) == ([], 0, V.END_EDGE)


def test_two_rooms_only_the_doors_cone_is_seen(lom):
    w, h, door_y, x0, y0 = 31, 21, 10, 12, 8
    plane = S.two_rooms(w, h, door_y)
    wall = w // 2
    plane[:, wall + 1:] = -1                                          # room B is unknown, so its seen cells are the viewpoint's set
    got = V.cast_fast(plane, [[x0, y0]], library_table(lom, 1024), V.params(1024, 40))
    seen = np.unpackbits(np.frombuffer(got["sets"][0].to_bytes((w * h + 7) // 8, "little"), np.uint8), bitorder="little")[:w * h]
    seen = seen.reshape(h, w).astype(bool)

    def angles(cx, cy):
        """the interval of directions from the start cell's centre to the cell (cx, cy)'s square (the cell lies to the right)"""
        a = [math.atan2(cy + sy - 0.5 - y0, cx + sx - 0.5 - x0) for sx in (0, 1) for sy in (0, 1)]
        return min(a), max(a)

    lo, hi = angles(wall, door_y)
    in_cone = np.zeros((h, w), bool)
    for cy in range(h):
        for cx in range(wall + 1, w):
            a, b = angles(cx, cy)
            in_cone[cy, cx] = a <= hi and b >= lo
    assert seen.sum() > 30 and not (seen & ~in_cone).any()
    assert got["records"][0]["unknown"] == seen.sum() and (~in_cone[:, wall + 1:]).sum() > 100


def test_depth_one_stops_at_the_first_unknown_cell(lom):
    table = library_table(lom, 4)
    plane = np.zeros((1, 9), np.int8)
    plane[0, 4:] = -1
    for depth, seen, d2, why in ((1, 5, 16, V.END_UNKNOWN), (3, 7, 36, V.END_UNKNOWN), (0, 9, 64, V.END_EDGE), (6, 9, 64, V.END_EDGE)):
        got = V.cast(plane, [[0, 0]], table, V.params(4, 20, 100, depth))
        assert got["records"][0]["seen"] == seen and got["beams"][0, 0] == (why << 24) | d2, depth
    # the start cell counts for no ray's depth
    got = V.cast(plane, [[4, 0]], table, V.params(4, 20, 100, 1))
    assert got["beams"][0, 0] == (V.END_UNKNOWN << 24) | 1 and got["records"][0].tolist() == (4, 0, 1, 6, 2, 4, 0, 0)


# ---- selection -----------------------------------------------------------------------------------------------------------------
def frontier_cast(lom, w=40, h=30, k=40, seed=3):
    from tests import regions_scenes as RS

    rng = np.random.default_rng(seed)
    plane = RS.frontier_plane(w, h, seed)
    vp = np.stack([rng.integers(0, w, k), rng.integers(0, h, k)], axis=1).astype(np.int32)
    return V.cast_fast(plane, vp, library_table(lom, 128), V.params(128, 8, 100, 3, V.KEEP_WINDOWS)), vp


def test_selection_properties(lom):
    got, vp = frontier_cast(lom)
    picks = V.select(got, V.select_params(12))
    assert len(picks) == 12 and len(set(picks["k"].tolist())) == 12
    union = 0
    for k in picks["k"]:
        union |= got["sets"][int(k)]
    assert int(picks["gain"].sum()) == bin(union).count("1")          # the marginal gains add up to the union
    assert (np.diff(picks["gain"].astype(np.int64)) <= 0).all()       # without costs the gains do not increase
    assert (picks["score"] == picks["gain"]).all() and picks["gain"][0] == got["records"]["unknown"].max()
    # ties go to the least index: a duplicate of the best viewpoint behind it never wins the first round
    best = int(picks["k"][0])
    twice = dict(got, sets=got["sets"] + [got["sets"][best]], records=np.concatenate([got["records"], got["records"][best:best + 1]]))
    again = V.select(twice, V.select_params(3))
    assert again["k"][0] == best and len(got["sets"]) not in again["k"].tolist()      # ... and then gains nothing
    # min_gain ends the selection early
    floor = int(picks["gain"][5])
    early = V.select(got, V.select_params(12, min_gain=floor + 1))
    assert 0 < len(early) <= 5 and early.tobytes() == picks[:len(early)].tobytes()
    assert len(V.select(got, V.select_params(12, min_gain=10 ** 6))) == 0
    # costs: a shift scales them, an unreached viewpoint is excluded, the score may be negative
    cost = (np.arange(len(vp), dtype=np.uint32) * 37) % 500
    cost[best] = V.UNREACHED
    priced = V.select(got, V.select_params(6, gain_weight=4, cost_shift=1), cost)
    assert best not in priced["k"].tolist()
    for e in priced:
        assert e["score"] == int(e["gain"]) * 4 - (int(cost[e["k"]]) >> 1)
    dear = V.select(got, V.select_params(2), np.full(len(vp), 1 << 20, np.uint32))
    assert len(dear) == 2 and (dear["score"] < 0).all() and dear["k"][0] == best
    assert V.select(got, V.select_params(0)) is None and V.select(got, V.select_params(1, 4097)) is None
    assert V.select(got, V.select_params(1, 1, 32)) is None and V.select(got, V.select_params(1, 1, 0, 0)) is None


# ---- the library's host side -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beams", [4, 5, 64, 360, 1000, 8192])
def test_direction_table_against_numpy(lom, beams):
    got, want = library_table(lom, beams), V.numpy_table(beams)
    assert got.dtype == np.int32 and got.shape == (beams, 2)
    assert np.abs(got.astype(np.int64) - want).max() <= 1
    assert got[0].tolist() == [32768, 0]
    if beams % 4 == 0:
        q = beams // 4
        assert got[q].tolist() == [0, 32768] and got[2 * q].tolist() == [-32768, 0] and got[3 * q].tolist() == [0, -32768]
    assert (np.abs(got).max(axis=1) >= 23170).all()                   # no direction is (0, 0)
    for bad in (0, 3, 8193):
        with pytest.raises(lom.LomError):
            lom.visibilityTable(bad)


def test_structures_and_symbols(lom):
    hdr = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    names = re.findall(r"\b(lom_visibility_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert len(names) == 20
    L = lom.capi.lib()
    for name in names:
        assert name in lom.capi.EXPORTED and hasattr(L, name), name
    assert C.sizeof(lom.capi.VisibilityParams) == 20 and C.sizeof(lom.capi.VisibilitySummary) == 40
    assert C.sizeof(lom.capi.VisibilitySelectParams) == 16 and C.sizeof(lom.capi.VisibilityCallStats) == 16
    assert lom.capi.VISIBILITY_RECORD == V.RECORD and lom.capi.VISIBILITY_PICK == V.PICK
    for name, value in (("KEEP_WINDOWS", V.KEEP_WINDOWS), ("KEEP_BEAMS", V.KEEP_BEAMS), ("END_INVALID", V.END_INVALID),
                        ("END_EDGE", V.END_EDGE), ("END_RANGE", V.END_RANGE), ("END_HIT", V.END_HIT), ("END_UNKNOWN", V.END_UNKNOWN),
                        ("END_CORNER", V.END_CORNER)):
        assert getattr(lom.capi, "VIS_" + name) == value
        assert re.search(r"LOM_VIS_%s\s*=\s*%d\b" % (name, value), hdr), name
    p = lom.visibilityParams(V.as_tuple(V.params(360, 31, 50, 5, 3)))
    assert (p.beams, p.range_cells, p.block_min, p.unknown_depth, p.flags) == (360, 31, 50, 5, 3)
    s = lom.visibilitySelectParams((16, 8, 2, 1))
    assert (s.n, s.gain_weight, s.cost_shift, s.min_gain) == (16, 8, 2, 1)
    assert hasattr(lom, "VisibilityGrid")
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for name in names:
        assert name in mirror, name
