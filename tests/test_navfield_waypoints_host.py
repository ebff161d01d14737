"""Line of sight and waypoints of the navigation field, the parts that need no GPU: the integer rule of
tests/navfield_waypoints_ref.py against a clip of the segment on exact fractions, the properties of the greedy on the
reference, the refusals that touch no device and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import navfield_waypoints_ref as Wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)
THRESHOLDS = (0, 50, 80)


def geo_of(w, h):
    return N.geometry(0.25, -3.0, 2.0, w, h)


def costs(rows):
    """cell costs from rows of 0 (blocked) / 1 (free), row 0 first"""
    return [[50 if v else 0 for v in row] for row in rows]


# ---- the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_integer_rule_equals_the_fraction_form(seed):
    rng = np.random.default_rng(500 + seed)
    mismatches, asymmetric, n = [], [], 0
    for k in range(10):
        w, h = ((1, 1), (13, 13), (1, 13), (13, 1))[seed] if k == 0 and seed < 4 else (int(v) for v in rng.integers(1, 14, 2))
        # cost bytes 0 .. 10 give cell costs 50 .. 80 under P0: the thresholds 50 and 80 cut through them
        plane = rng.integers(0, 11, (h, w)).astype(np.int8)
        plane[rng.random((h, w)) < (0.0, 0.1, 0.25, 0.4)[seed % 4]] = 100
        c = N.costs_of(plane, P0)
        for _ in range(30):
            a = (int(rng.integers(-1, w + 1)), int(rng.integers(-1, h + 1)))
            b = (int(rng.integers(-1, w + 1)), int(rng.integers(-1, h + 1)))
            for t in THRESHOLDS:
                got, want = Wr.visible(c, w, h, a, b, t), Wr.visible_by_fractions(c, w, h, a, b, t)
                n += 1
                if got != want:
                    mismatches.append((w, h, a, b, t, got, want))
                # symmetric wherever both ends are clear (the end a walk starts from is not read)
                inside = 0 <= a[0] < w and 0 <= a[1] < h and 0 <= b[0] < w and 0 <= b[1] < h
                if inside and Wr.clear(c[a[1]][a[0]], t) and Wr.clear(c[b[1]][b[0]], t) and got != Wr.visible(c, w, h, b, a, t):
                    asymmetric.append((w, h, a, b, t))
    assert n == 900 and not mismatches and not asymmetric, (mismatches[:5], asymmetric[:5])


def test_corner_cases_by_hand():
    both = lambda c, w, h, a, b, t=0: (Wr.visible(c, w, h, a, b, t), Wr.visible_by_fractions(c, w, h, a, b, t))
    free = costs([[1] * 4] * 4)
    assert both(free, 4, 4, (0, 0), (3, 3)) == (True, True) and both(free, 4, 4, (3, 0), (0, 3)) == (True, True)
    # an exact diagonal past one blocked side cell, on either side, and past two
    for blocked in ([(1, 0)], [(0, 1)], [(2, 1)], [(1, 0), (0, 1)], [(2, 3), (3, 2)]):
        rows = [[1] * 4 for _ in range(4)]
        for x, y in blocked:
            rows[y][x] = 0
        c = costs(rows)
        assert both(c, 4, 4, (0, 0), (3, 3)) == (False, False), blocked
        assert both(c, 4, 4, (3, 3), (0, 0)) == (False, False), blocked
    # ... a blocked cell that the diagonal neither crosses nor touches does not matter
    rows = [[1] * 4 for _ in range(4)]
    rows[0][2] = rows[3][0] = 0
    assert both(costs(rows), 4, 4, (0, 0), (3, 3)) == (True, True)
    # a corner passed on a slope other than 1: the segment (0, 0) -> (2, 6) runs through the lattice point (1, 2)
    rows = [[1] * 3 for _ in range(7)]
    assert both(costs(rows), 3, 7, (0, 0), (2, 6)) == (True, True)
    rows[2][0] = 0                                                       # the cell (0, 2), beside that corner
    assert both(costs(rows), 3, 7, (0, 0), (2, 6)) == (False, False)
    assert both(costs(rows), 3, 7, (0, 0), (1, 2)) == (True, True)
    # dx == 0, dy == 0, A == B
    line = costs([[1, 1, 0, 1, 1]])
    assert both(line, 5, 1, (0, 0), (1, 0)) == (True, True) and both(line, 5, 1, (0, 0), (3, 0)) == (False, False)
    assert both(line, 5, 1, (4, 0), (3, 0)) == (True, True) and both(line, 5, 1, (4, 0), (1, 0)) == (False, False)
    col = costs([[1], [1], [0], [1]])
    assert both(col, 1, 4, (0, 0), (0, 1)) == (True, True) and both(col, 1, 4, (0, 3), (0, 0)) == (False, False)
    assert both(line, 5, 1, (1, 0), (1, 0)) == (True, True)
    assert both(line, 5, 1, (2, 0), (2, 0)) == (True, True)              # A == B on a blocked cell: A is tested for nothing
    # B blocked: not visible; A blocked: visible, A is not read
    assert both(line, 5, 1, (1, 0), (2, 0)) == (False, False) and both(line, 5, 1, (2, 0), (1, 0)) == (True, True)
    assert both(line, 5, 1, (2, 0), (4, 0)) == (True, True)
    # outside the grid
    for a, b in (((-1, 0), (0, 0)), ((0, 0), (5, 0)), ((0, 1), (0, 0)), ((0, 0), (0, -1)), ((7, 7), (7, 7))):
        assert both(line, 5, 1, a, b) == (False, False)
    # the threshold: a cell above it blocks, one at it does not
    c = [[50, 80, 81, 50]]
    assert both(c, 4, 1, (0, 0), (1, 0), 80) == (True, True) and both(c, 4, 1, (0, 0), (2, 0), 80) == (False, False)
    assert both(c, 4, 1, (0, 0), (3, 0), 0) == (True, True) and both(c, 4, 1, (0, 0), (1, 0), 50) == (False, False)


def test_an_allowed_step_is_always_visible():
    rng = np.random.default_rng(9)
    n = 0
    for _ in range(20):
        w, h = (int(v) for v in rng.integers(1, 14, 2))
        c = N.costs_of(S.random_plane(rng, w, h), P1)
        for y in range(h):
            for x in range(w):
                for dx, dy, _ln in N.STEPS:
                    if c[y][x] and N.allowed(c, w, h, x, y, dx, dy):
                        n += 1
                        assert Wr.visible(c, w, h, (x, y), (x + dx, y + dy), 0)
    assert n > 1000


# ---- the greedy, on the reference ----------------------------------------------------------------------------------------------
def solved(w, h, plane, p, goals):
    geo = geo_of(w, h)
    return geo, N.solve(geo, plane, p, np.array(goals))


def is_subsequence(short, long):
    it = iter(long)
    return all(any(v == u for u in it) for v in short)


def test_greedy_properties():
    rng = np.random.default_rng(4)
    for w, h, plane, p in ((33, 31, S.random_plane(rng, 33, 31, obstacles=0.12), P1), (40, 40, S.diagonal_gaps(40, 40), P0),
                           (30, 20, S.pocket(30, 20), P0), (25, 25, S.spiral(25, 25), P0), (40, 21, S.serpentine(40, 21), P0)):
        free = np.argwhere((plane >= 0) & (plane <= 90))
        geo, r = solved(w, h, plane, p, [tuple(free[0][::-1])])
        c = r["costs"]
        for s in [tuple(int(v) for v in f[::-1]) for f in free[:: max(1, len(free) // 25)]]:
            route = N.path(geo, c, r["P"], s)
            for t in (0, 50, 65):
                see = lambda a, b: Wr.visible(c, w, h, a, b, t)
                assert Wr.shortcut(route, 1, see) == route                       # W = 1: the route, whatever the threshold
                for W in (2, 7, 65535):
                    wp = Wr.shortcut(route, W, see)
                    if not route:
                        assert wp == []
                        continue
                    assert wp[0] == route[0] and wp[-1] == route[-1] and is_subsequence(wp, route)
                    at = [route.index(v) for v in wp]                            # (a route never visits a cell twice)
                    assert all(0 < b - a <= W for a, b in zip(at, at[1:]))
                    assert all(see(route[a], route[b]) for a, b in zip(at, at[1:]) if b - a > 1)
                    # never longer than the route: a shortcut replaces a piece by its chord
                    assert Wr.polyline_cells(wp) <= Wr.polyline_cells(route) + 1e-9


def test_open_ground_gives_two_waypoints():
    w, h = 40, 23
    geo, r = solved(w, h, S.empty(w, h), P0, [(31, 17)])
    c = r["costs"]
    see = lambda a, b: Wr.visible(c, w, h, a, b, 0)
    for s in ((0, 0), (39, 0), (0, 22), (5, 17), (31, 0), (12, 20)):
        route = N.path(geo, c, r["P"], s)
        n = len(route)
        assert n > 2
        for W in (n - 1, n, 65535):
            assert Wr.shortcut(route, W, see) == [route[0], route[-1]]
        assert len(Wr.shortcut(route, n - 2, see)) == 3
    assert Wr.shortcut([(31, 17)], 5, see) == [(31, 17)] and Wr.shortcut([], 5, see) == []
    cells, counts, lengths = Wr.waypoints(geo, c, r["P"], np.array([(0, 0), (31, 17), (-1, 3), (39, 22)]), 0, 65535, 10, 3)
    assert counts.tolist() == [2, 1, 0, 2] and lengths[1] == 1 and lengths[2] == 0 and lengths[0] > 10
    assert cells[0].tolist() == [[0, 0], list(N.path(geo, c, r["P"], (0, 0))[9]), [0, 0]]      # the route was cut at route_cap
    assert cells[1].tolist() == [[31, 17], [0, 0], [0, 0]] and (cells[2] == 0).all()


# ---- refusals and declarations -------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(lom):
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    starts, cells = np.zeros((2, 2), np.int32), np.full((2, 4, 2), 7, np.uint16)
    counts, lengths = np.full(2, 7, np.uint32), np.full(2, 7, np.uint32)
    out, pairs = np.full(3, 7, np.uint8), np.zeros((3, 4), np.int32)
    for p in ((0, 64, 100, 0), (0, 0, 100, 0), (0, 65536, 100, 0), (0, 64, 0, 0), (0, 64, 100, 1)):
        prm = lom.navfieldWaypointParams(p)
        assert L.lom_navfield_waypoints(None, 0, starts.ctypes.data, 2, C.byref(prm), cells.ctypes.data, 4, counts.ctypes.data,
                                        lengths.ctypes.data) == ERR_ARG
    assert L.lom_navfield_waypoints(None, 0, None, 0, None, None, 0, None, None) == ERR_ARG
    assert L.lom_navfield_visible(None, pairs.ctypes.data, 3, 0, out.ctypes.data) == ERR_ARG
    assert L.lom_navfield_visible(None, None, 0, 0, None) == ERR_ARG
    assert (cells == 7).all() and (counts == 7).all() and (lengths == 7).all() and (out == 7).all()
    with pytest.raises(TypeError):
        lom.navfieldWaypointParams((0, 64, 100))
    p = lom.navfieldWaypointParams(dict(max_cell_cost=50, lookahead=64, route_cap=100, flags=0))
    assert (p.max_cell_cost, p.lookahead, p.route_cap, p.flags) == (50, 64, 100, 0)


def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in ("lom_navfield_waypoints", "lom_navfield_visible"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"LOM_NAV_OPT_TEST_SHORTCUT_SERIAL\s*=\s*5", text) and lom.capi.NAV_OPT_TEST_SHORTCUT_SERIAL == 5
    assert re.search(r"\*\s+8\. Line of sight\.", text) and re.search(r"\*\s+9\. Waypoints\.", text)
    assert C.sizeof(lom.capi.NavFieldWaypointParams) == 16
    assert [k for k, _ in lom.capi.NavFieldWaypointParams._fields_] == ["max_cell_cost", "lookahead", "route_cap", "flags"]
    fields = re.search(r"typedef struct \{([^}]*)\} lom_navfield_waypoint_params;", text).group(1)
    assert re.findall(r"uint32_t (\w+);", fields) == ["max_cell_cost", "lookahead", "route_cap", "flags"]
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for name in ("waypoints", "visible", "waypointsMetres", "polylineLength"):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert hasattr(lom.NavField, name), name
    assert re.search(r"\bnavfieldWaypointParams\s*\(", mirror) and hasattr(lom, "navfieldWaypointParams")
    assert lom.capi.lib().lom_abi_version() == 2
