"""Navigation field, the parts that need no GPU: the reference (tests/navfield_ref.py) against scipy's Dijkstra on the same
graph and against a brute-force Bellman-Ford, its paths, the cell-cost table against the library's, two scenes on the
reference alone, the declarations and the refusals that touch no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import navfield_ref as N
from tests import navfield_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_navfield_create", "lom_navfield_destroy", "lom_navfield_last_error", "lom_navfield_clear",
               "lom_navfield_get_geometry", "lom_navfield_stream", "lom_navfield_device", "lom_navfield_wait_event",
               "lom_navfield_set_option", "lom_navfield_solve", "lom_navfield_solve_device", "lom_navfield_solve_from_clearance",
               "lom_navfield_potential", "lom_navfield_potential_device", "lom_navfield_paths", "lom_navfield_query",
               "lom_navfield_cell_costs", "lom_navfield_stats"]
P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)


def geo_of(w, h):
    return N.geometry(0.25, -3.0, 2.0, w, h)


def graph_edges(c, w, h):
    """the directed steps a -> b as (a, b, weight) with cells numbered row-major"""
    out = []
    for y in range(h):
        for x in range(w):
            if c[y][x]:
                for dx, dy, ln in N.STEPS:
                    if N.allowed(c, w, h, x, y, dx, dy):
                        out.append((y * w + x, (y + dy) * w + x + dx, ln * c[y][x]))
    return out


# ---- the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_reference_equals_scipy_dijkstra(seed):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import csr_matrix

    rng = np.random.default_rng(seed)
    w, h = (int(v) for v in rng.integers(1, 40, 2))
    plane = S.random_plane(rng, w, h, obstacles=(0.0, 0.1, 0.3, 0.3, 0.5, 0.3)[seed])
    p = P1 if seed % 2 else P0
    goals = np.stack([rng.integers(-1, w + 1, 4), rng.integers(-1, h + 1, 4)], axis=1)
    r = N.solve(geo_of(w, h), plane, p, goals)
    c = r["costs"]
    e = graph_edges(c, w, h)
    used = sorted({gy * w + gx for gx, gy in goals if 0 <= gx < w and 0 <= gy < h and c[gy][gx]})
    assert r["summary"]["goals_used"] == len(used) and r["summary"]["goals_used"] + r["summary"]["goals_rejected"] <= 4
    want = np.full(w * h, np.inf)
    if used:
        # P[a] is the distance from a to the nearest goal: Dijkstra from the goals over the reversed steps
        m = csr_matrix(([float(v[2]) for v in e], ([v[1] for v in e], [v[0] for v in e])), shape=(w * h, w * h))
        want = csgraph.dijkstra(m, directed=True, indices=used, min_only=True) if e else np.where(np.isin(np.arange(w * h), used), 0.0, np.inf)
    got = r["P"].ravel()
    assert np.array_equal(got == N.UNREACHED, np.isinf(want))
    assert np.array_equal(got[got != N.UNREACHED].astype(np.float64), want[~np.isinf(want)])   # (integers below 2^53: exact)
    s = r["summary"]
    assert s["cells_blocked"] + s["cells_reached"] + s["cells_unreached"] == w * h and s["range_exceeded"] == 0


@pytest.mark.parametrize("seed", range(8))
def test_reference_equals_brute_force_bellman_ford(seed):
    rng = np.random.default_rng(100 + seed)
    w, h = int(rng.integers(1, 13)), int(rng.integers(1, 10))
    plane = S.random_plane(rng, w, h, obstacles=0.25, unknown=0.15)
    p = P1 if seed % 2 else P0
    goals = np.stack([rng.integers(0, w, 2), rng.integers(0, h, 2)], axis=1)
    r = N.solve(geo_of(w, h), plane, p, goals)
    c = r["costs"]
    e = graph_edges(c, w, h)
    P = [N.UNREACHED] * (w * h)
    for gx, gy in goals:
        if c[gy][gx]:
            P[gy * w + gx] = 0
    for _ in range(w * h):
        changed = False
        for a, b, wt in e:
            if P[b] != N.UNREACHED and P[b] + wt <= N.MAX and P[b] + wt < P[a]:
                P[a], changed = P[b] + wt, True
        if not changed:
            break
    assert [int(v) for v in r["P"].ravel()] == P


def check_paths(geo, r, starts):
    c, P = r["costs"], r["P"]
    for s in starts:
        route = N.path(geo, c, P, s)
        if s is None or P[s[1], s[0]] == N.UNREACHED:
            assert route == []
            continue
        assert route[0] == tuple(s) and P[route[-1][1], route[-1][0]] == 0
        assert N.path_weight(c, route) == int(P[s[1], s[0]])
        for (ax, ay), (bx, by) in zip(route, route[1:]):
            assert N.allowed(c, geo["width"], geo["height"], ax, ay, bx - ax, by - ay)
        assert len(set(route)) == len(route)


def test_paths_sum_to_the_potential_and_use_allowed_steps():
    rng = np.random.default_rng(5)
    for w, h, plane in ((33, 31, S.random_plane(rng, 33, 31)), (40, 21, S.serpentine(40, 21)), (25, 25, S.spiral(25, 25)),
                        (40, 40, S.diagonal_gaps(40, 40)), (30, 20, S.pocket(30, 20))):
        geo = geo_of(w, h)
        free = np.argwhere(plane == 0)
        goals = [tuple(int(v) for v in free[0][::-1]), tuple(int(v) for v in free[len(free) // 2][::-1])]
        r = N.solve(geo, plane, P0, np.array(goals))
        assert r["summary"]["goals_used"] >= 1
        starts = [(int(x), int(y)) for y, x in free[:: max(1, len(free) // 60)]] + [None, goals[0]]
        check_paths(geo, r, starts)
        cells, lengths = N.paths(geo, r["costs"], r["P"], np.array([s if s else (-1, -1) for s in starts]), 7)
        assert lengths[-1] == 1 and lengths[-2] == 0 and (cells[-2] == 0).all() and tuple(cells[-1, 0]) == tuple(goals[0])
    # the pocket's inside is passable and unreached; the serpentine visits every corridor cell
    r = N.solve(geo_of(30, 20), S.pocket(30, 20), P0, np.array([(0, 0)]))
    assert r["summary"]["cells_unreached"] > 0 and r["P"][20 // 3 + 1, 30 // 3 + 1] == N.UNREACHED
    r = N.solve(geo_of(40, 21), S.serpentine(40, 21), P0, np.array([(0, 0)]))
    free = int((S.serpentine(40, 21) == 0).sum())                 # one route through all of them, axial steps only
    assert r["summary"]["cells_unreached"] == 0 and r["summary"]["max_potential"] == 5 * 50 * (free - 1)


def test_no_corner_is_cut():
    # two obstacles that touch at a corner: the diagonal between them is not a step
    plane = np.zeros((3, 3), np.int8)
    plane[0, 1] = plane[1, 0] = 100
    r = N.solve(geo_of(3, 3), plane, N.params(1, 0, 1, 98), np.array([(0, 0)]))
    assert (r["P"] == np.array([[0, N.UNREACHED, N.UNREACHED], [N.UNREACHED] * 3, [N.UNREACHED] * 3], np.uint32)).all()
    plane[0, 1] = 0
    r = N.solve(geo_of(3, 3), plane, N.params(1, 0, 1, 98), np.array([(0, 0)]))
    assert r["P"][1, 1] == 10 and r["P"][0, 1] == 5 and r["P"][1, 2] == 12    # (1, 1) goes round: N is blocked, so E then N


def test_values_by_hand_and_the_range():
    geo = geo_of(4, 1)
    plane = np.array([[0, 10, -1, 98]], np.int8)
    r = N.solve(geo, plane, N.params(2, 3, 7, 98, N.UNKNOWN_PASSABLE), np.array([(0, 0), (0, 0), (9, 0)]))
    assert r["P"].tolist() == [[0, 5 * 32, 5 * 32 + 5 * 7, 5 * 32 + 5 * 7 + 5 * 296]]     # a step pays for the cell it leaves
    assert r["summary"] == dict(cells_blocked=0, cells_reached=4, cells_unreached=0, cells_invalid=0, goals_used=1, goals_rejected=1,
                                range_exceeded=0, max_potential=1675)
    r = N.solve(geo, plane, N.params(2, 3, 7, 98), np.array([(0, 0)]))
    assert r["P"].tolist() == [[0, 160, N.UNREACHED, N.UNREACHED]] and r["summary"]["cells_blocked"] == 1 and r["summary"]["cells_unreached"] == 1
    assert N.solve(geo, plane, N.params(0, 3, 7, 98), np.array([(0, 0)]))["error"]
    # the range: at the largest cell cost a straight corridor passes LOM_NAV_MAX after 51 steps
    big = N.params(N.MAX_CELL_COST, 0, 1, 98)
    r = N.solve(geo_of(70, 1), S.empty(70, 1), big, np.array([(0, 0)]))
    steps = N.MAX // (5 * N.MAX_CELL_COST)
    assert steps == 51 and r["summary"]["range_exceeded"] == 1 and r["summary"]["cells_unreached"] == 70 - 52
    assert r["P"][0, 51] == 51 * 5 * N.MAX_CELL_COST and r["P"][0, 52] == N.UNREACHED
    # the rule is about steps, not cells: on 52 cells all are reached, but the step from cell 50 back to cell 51 would pass
    # the range, so the flag is up; on 51 cells no step does
    s52 = N.solve(geo_of(52, 1), S.empty(52, 1), big, np.array([(0, 0)]))["summary"]
    assert s52["range_exceeded"] == 1 and s52["cells_unreached"] == 0
    assert N.solve(geo_of(51, 1), S.empty(51, 1), big, np.array([(0, 0)]))["summary"]["range_exceeded"] == 0
    # invalid bytes are impassable and counted
    r = N.solve(geo, np.array([[0, 101, -2, 0]], np.int8), P1, np.array([(0, 0)]))
    assert r["summary"]["cells_invalid"] == 2 and r["summary"]["cells_blocked"] == 2 and r["summary"]["cells_unreached"] == 1
    # metres: the floor rule at cell borders
    assert N.cells_of(geo, [[-3.0, 2.0], [-2.75, 2.0], [-2.7500002, 2.24], [-3.0000002, 2.0], [-2.0, 2.25], [np.nan, 2.0]], True) == \
        [(0, 0), (1, 0), (0, 0), None, None, None]


# ---- scenes, on the reference alone ---------------------------------------------------------------------------------------------
def test_every_path_from_the_far_room_passes_the_door():
    w, h, door = 41, 23, 6
    plane = S.two_rooms(w, h, door)
    geo = geo_of(w, h)
    r = N.solve(geo, plane, P0, np.array([(3, 17)]))
    assert r["summary"]["cells_unreached"] == 0
    for y in range(h):
        for x in range(w // 2 + 1, w, 3):
            assert (w // 2, door) in N.path(geo, r["costs"], r["P"], (x, y))
    for x in range(0, w // 2, 4):
        assert (w // 2, door) not in N.path(geo, r["costs"], r["P"], (x, 2))


def test_a_path_keeps_to_the_middle_of_a_wide_corridor():
    """A corridor 15 cells wide between two walls, its cost inflated by tests/clearance_ref.py.  With factor > 0 the path
    between two points near one wall moves to the middle row and stays there; with factor == 0 it stays beside the wall."""
    w, h, res = 120, 17, 0.25
    occ = np.zeros((h, w), np.int8)
    occ[0, :] = occ[-1, :] = 100
    cgeo = K.geometry(res, 0.0, 0.0, w, h)
    cost = K.update(cgeo, occ, None, K.params(inflation_radius=2.0, inscribed_radius=0.25, decay=1.0))["cost"]
    assert cost[h // 2, 5] < cost[2, 5] < cost[1, 5] == 99
    geo = N.geometry(res, 0.0, 0.0, w, h)
    start, goal = (2, 2), (w - 3, 2)
    r = N.solve(geo, cost, N.params(10, 20, 1, 98), np.array([goal]))
    route = N.path(geo, r["costs"], r["P"], start)
    rows = [y for x, y in route if 20 <= x < w - 20]
    assert rows and set(rows) == {h // 2}
    r0 = N.solve(geo, cost, N.params(10, 0, 1, 98), np.array([goal]))
    rows0 = [y for x, y in N.path(geo, r0["costs"], r0["P"], start)]
    assert max(rows0) < h // 2


# ---- declarations and refusals -----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"navigation field", text)
    assert re.search(r"#define LOM_NAV_UNREACHED 0xFFFFFFFFu", text) and re.search(r"#define LOM_NAV_MAX 0xFFFFFFFEu", text)
    for name, value in dict(LOM_NAV_UNKNOWN_PASSABLE=1, LOM_NAV_METRES=1, LOM_NAV_OPT_TEST_INNER_CAP=1, LOM_NAV_OPT_TEST_BATCH=2,
                            LOM_NAV_OPT_TEST_ALL_TILES=3).items():
        assert re.search(r"%s\s*=\s*%d" % (name, value), text), name
    assert lom.capi.lib().lom_abi_version() == 2
    assert (lom.capi.NAV_UNREACHED, lom.capi.NAV_MAX, lom.capi.NAV_UNKNOWN_PASSABLE) == (N.UNREACHED, N.MAX, N.UNKNOWN_PASSABLE)
    for name, size in dict(NavFieldParams=20, NavFieldSummary=64, NavFieldSolveStats=24).items():
        assert C.sizeof(getattr(lom.capi, name)) == size, name
    assert [k for k, _ in lom.capi.NavFieldSummary._fields_] == list(N.SUMMARY_KEYS)
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    assert re.search(r"class NavField", mirror) and re.search(r"\bnavfieldParams\s*\(", mirror)
    for name in ("solve", "solveFromClearance", "potential", "paths", "query", "clear", "setOption", "stats"):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert hasattr(lom.NavField, name), name
    assert lom.navfieldParams((5, 1, 9, 98, 1)).max_passable == 98


@pytest.mark.parametrize("p", [(1, 0, 0, 0, 0), (50, 3, 400, 98, 0), (50, 3, 400, 90, 1), ((1 << 24) - 1, 0, (1 << 24) - 1, 98, 1),
                               (1, 171195, 1, 98, 0), (7, 11, 0xFFFFFFFF, 40, 0)])
def test_cell_costs_of_the_library(lom, p):
    got = lom.navfieldCellCosts(p)
    want = N.cell_costs(N.params(*p))
    assert N.params_ok(N.params(*p)) and got.dtype == np.uint32 and len(got) == 256
    for b in range(256):
        assert int(got[b]) == want[b], b
    assert all(v == 0 for v in want[p[3] + 1:255]) and (want[255] != 0) == bool(p[4] & 1)


def test_bad_arguments_are_refused_without_a_device(lom):
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    out = np.full(256, 7, np.uint32)
    for bad in ((0, 0, 1, 98, 0), (1, 0, 1, 99, 0), (1, 0, 1, -1, 0), (1, 0, 1, 100, 0), (1, 171197, 1, 98, 0), (1 << 24, 0, 1, 98, 0),
                (1, 0xFFFFFFFF, 1, 98, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1, 0, 0), (5, 1, 0, 98, 1), (5, 1, 1 << 24, 98, 1), (5, 1, 1, 98, 2),
                (5, 1, 1, 98, 3)):
        assert L.lom_navfield_cell_costs(C.byref(lom.navfieldParams(bad)), out.ctypes.data) == ERR_ARG, bad
        assert not N.params_ok(N.params(*bad)), bad
        with pytest.raises(lom.LomError):
            lom.navfieldCellCosts(bad)
    assert (out == 7).all()
    assert L.lom_navfield_cell_costs(None, out.ctypes.data) == ERR_ARG
    assert L.lom_navfield_cell_costs(C.byref(lom.navfieldParams((5, 1, 1, 98, 0))), None) == ERR_ARG
    h = C.c_void_p()
    good = dict(resolution=0.25, origin_x=0.0, origin_y=0.0, width=10, height=10)
    for change in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=np.nan), dict(resolution=np.inf),
                   dict(origin_x=np.nan), dict(origin_y=np.inf), dict(width=0), dict(height=0), dict(width=8193), dict(height=8193)):
        geo = lom.capi.OccupancyGeometry(**dict(good, **change))
        assert L.lom_navfield_create(C.byref(geo), 0, C.byref(h)) == ERR_ARG, change
        assert b"geometry" in L.lom_navfield_last_error(None)
    assert L.lom_navfield_create(None, 0, C.byref(h)) == ERR_ARG
    assert L.lom_navfield_create(C.byref(lom.capi.OccupancyGeometry(**good)), 0, None) == ERR_ARG
    # NULL handles; the summary is zeroed
    prm, plane, goal = lom.navfieldParams((5, 1, 1, 98, 0)), np.zeros(100, np.int8), np.zeros(2, np.int32)
    sm = lom.capi.NavFieldSummary()

    def zeroed(rc):
        ok = rc == ERR_ARG and sm.asdict() == dict.fromkeys(N.SUMMARY_KEYS, 0)
        sm.cells_blocked = sm.max_potential = 5
        return ok

    sm.cells_blocked = sm.max_potential = 5
    assert zeroed(L.lom_navfield_solve(None, plane.ctypes.data, C.byref(prm), 0, goal.ctypes.data, 1, C.byref(sm)))
    assert zeroed(L.lom_navfield_solve_device(None, None, None, C.byref(prm), 0, goal.ctypes.data, 1, C.byref(sm)))
    assert zeroed(L.lom_navfield_solve_from_clearance(None, None, C.byref(prm), 0, goal.ctypes.data, 1, C.byref(sm)))
    assert L.lom_navfield_potential(None, None, 0) == ERR_ARG and L.lom_navfield_potential_device(None, C.byref(h)) == ERR_ARG
    assert L.lom_navfield_paths(None, 0, None, 0, None, 0, None) == ERR_ARG and L.lom_navfield_query(None, None, 0, None) == ERR_ARG
    assert L.lom_navfield_stats(None, None) == ERR_ARG
    assert L.lom_navfield_clear(None) == ERR_ARG and L.lom_navfield_device(None) == ERR_ARG
    assert L.lom_navfield_get_geometry(None, None) == ERR_ARG and L.lom_navfield_wait_event(None, None) == ERR_ARG
    assert L.lom_navfield_set_option(None, 1, 1) == ERR_ARG and L.lom_navfield_stream(None) is None
    L.lom_navfield_destroy(None)
    with pytest.raises(TypeError):
        lom.navfieldParams(dict(neutral=1))  # no defaults: all five fields or none
