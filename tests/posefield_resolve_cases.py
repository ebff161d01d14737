"""The case table of the pose field's re-solve, shared by tests/test_posefield_resolve_host.py (which asserts on the reference
alone that no case is vacuous) and tests/test_posefield_resolve_gpu.py (which runs every case on the device).  A case is a
dict: name, w, h, kept (the plane of the solve), p, fp (footprint), goals, new (the plane of the re-solve), window, tags.
Tags: "raises" (the least raised set is not empty), "lowers" (some state's P falls), "degenerate" (the three cases that may
change no state) and "outside" (a window wholly outside the grid: nothing can change)."""
import numpy as np

from tests import navfield_ref as N
from tests import posefield_ref as R
from tests import posefield_resolve_ref as Q
from tests import posefield_scenes as S

RES, ORIGIN = 0.25, (-3.0, 2.0)
NAV = N.params(50, 3, 400, 98)
BOTH = R.SPIN | R.REVERSE
P_NONE = R.params(NAV, 20, 1, 200, 0)
P_BOTH = R.params(NAV, 20, 1, 200, BOTH)               # spin_cost 1: a chain of spins is the cheapest supporter
P_DOOR = R.params(NAV, 20, 30, 200, 0)
TILE = (32, 8)
# under one tile, exactly one, four tiles with one-cell remainders, 3 x 3 tiles (one with all eight neighbours), the doorway
SHAPES = [(1, 1), (1, 20), (40, 1), (31, 7), (32, 8), (33, 9), (65, 17), (48, 32)]
BIG = S.big(np.random.default_rng(3))
_REFS, _CASES = {}, {}


def geo_of(w, h):
    return N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)


def put(plane, cells, value):
    """a copy with the cells (x, y) that exist set"""
    out = plane.copy()
    for x, y in cells:
        if 0 <= x < out.shape[1] and 0 <= y < out.shape[0]:
            out[y, x] = value
    return out


def goals_on(plane, p, fp, n=3):
    """goals spread over the passable states of a plane: the first names its cell under h = -1, the others one state each"""
    states = np.argwhere(R.layers(plane, p, R.stencils(fp)) != 0)
    if not len(states):
        return np.array([(0, 0, -1)], np.int32)
    pick = states[np.unique(((np.arange(n) + 1) * len(states)) // (n + 1))]
    return np.array([(x, y, -1 if k == 0 else hd) for k, (hd, y, x) in enumerate(pick.tolist())], np.int32)


def _generic(w, h, fp_name, fp, p, flags_name):
    """the cases every shape runs, per footprint and flags"""
    rng = np.random.default_rng(1000 * w + h)
    rnd = S.sparse(rng, w, h, 0.02)
    if (rnd == 100).all():
        rnd[:] = 5                                        # (the one cell of the smallest grid)
    free = rnd != 100
    other, dearer, cheaper = rnd.copy(), rnd.copy(), rnd.copy()
    other[free] = ((rnd[free].astype(int) + 7) % 41).astype(np.int8)
    dearer[free] = (rnd[free].astype(int) + 25).astype(np.int8)
    cheaper[free] = np.maximum(rnd[free].astype(int) - 25, 0).astype(np.int8)
    goals = goals_on(rnd, p, fp)
    quarter = (w // 4, h // 4, max(w // 2, 1), max(h // 2, 1))
    wall = put(rnd, [(w // 2, y) for y in range(h)] if w > 1 else [(0, h // 2)], 100)
    blocked = put(rnd, [(0, 0)], 100)
    out = {
        "null_window": (rnd, goals, other, None, ()),
        "window_outside": (rnd, goals, other, (w, 0, 5, 5), ("outside",)),
        "costs_raised": (rnd, goals, dearer, quarter, ()),
        "costs_lowered": (rnd, goals, cheaper, quarter, ()),
        "wall_put": (rnd, goals, wall, (w // 2, 0, 1, h), ()),
        "wall_taken": (wall, goals_on(wall, p, fp), rnd, (w // 2 - 1, -3, 3, h + 9), ()),
        "edge_cells": (rnd, goals, put(put(rnd, [(w - 1, h - 1)], 100), [(0, h - 1), (w - 1, 0)], 77), None, ()),
        "same_plane": (rnd, goals, rnd, quarter, ("degenerate",)),
        "wall_to_99": (blocked, goals_on(blocked, p, fp), put(blocked, [(0, 0)], 99), (0, 0, 1, 1), ("degenerate",)),
        "all_blocked": (rnd, goals, S.all_blocked(w, h), None, ("degenerate",)),
    }
    return [dict(name=f"{w}x{h}/{fp_name}/{flags_name}/{k}", w=w, h=h, kept=v[0], p=p, fp=fp, goals=v[1], new=v[2], window=v[3],
                 tags=set(v[4])) for k, v in out.items()]


def _named():
    """the cases that are about one thing each"""
    out = []

    def case(name, w, h, kept, p, fp, goals, new, window, *tags):
        out.append(dict(name=name, w=w, h=h, kept=kept, p=p, fp=fp, goals=np.array(goals, np.int32).reshape(-1, 3), new=new, window=window,
                        tags=set(tags)))

    # the serpentine: one route through every tile; a one-cell corridor is turned in by spins only
    w, h = 65, 17
    serp = S.serpentine(w, h)
    cut = put(serp, [(w // 2, 4)], 100)
    case("serpentine_route_blocked", w, h, serp, P_BOTH, S.POINT, [(0, 0, -1)], cut, (w // 2, 4, 1, 1), "raises")
    case("serpentine_route_freed", w, h, cut, P_BOTH, S.POINT, [(0, 0, -1)], serp, (w // 2, 4, 1, 1), "lowers")
    # costs over a quarter, every footprint
    rng = np.random.default_rng(17)
    rnd = S.sparse(rng, w, h, 0.01)
    free = rnd != 100
    dearer, cheaper = rnd.copy(), rnd.copy()
    dearer[free] = (rnd[free].astype(int) + 25).astype(np.int8)
    cheaper[free] = np.maximum(rnd[free].astype(int) - 25, 0).astype(np.int8)
    quarter = (w // 4, h // 4, w // 2, h // 2)
    for fp_name, fp in (("point", S.POINT), ("9x3", S.RECT_9x3), ("L", S.L_SHAPE), ("1024", BIG)):
        for flags_name, p in (("none", P_NONE), ("both", P_BOTH)):
            goals = goals_on(rnd, p, fp, 2)
            case(f"quarter_raised/{fp_name}/{flags_name}", w, h, rnd, p, fp, goals, dearer, quarter, "raises")
            case(f"quarter_lowered/{fp_name}/{flags_name}", w, h, rnd, p, fp, goals, cheaper, quarter, "lowers")
    # the doorway, both footprints: closing one of the three door cells leaves the point a way and the rectangle none
    dw, dh = 48, 32
    door, _ = S.doorway(dw, dh, 3)
    shut = put(door, [(24, 17)], 100)
    for fp_name, fp in (("point", S.POINT), ("9x3", S.RECT_9x3)):
        case(f"door_closed/{fp_name}", dw, dh, door, P_DOOR, fp, [(43, 16, -1)], shut, (24, 17, 1, 1), *(("raises",) if fp_name == "9x3" else ()))
        case(f"door_opened/{fp_name}", dw, dh, shut, P_DOOR, fp, [(43, 16, -1)], door, (24, 17, 1, 1), *(("lowers",) if fp_name == "9x3" else ()))
    # changed cells whose dilated boxes cross a tile corner: x = 31 .. 33, y = 7 .. 9
    for (cw, ch) in ((33, 9), (65, 17)):
        base = S.sparse(np.random.default_rng(cw), cw, ch, 0.0)
        corner = [(x, y) for x in (31, 32, 33) for y in (7, 8, 9)]
        for fp_name, fp in (("point", S.POINT), ("9x3", S.RECT_9x3), ("L", S.L_SHAPE)):
            for flags_name, p in (("none", P_NONE), ("both", P_BOTH)):
                goals = goals_on(base, p, fp, 2)
                case(f"tile_corner_blocked/{cw}x{ch}/{fp_name}/{flags_name}", cw, ch, base, p, fp, goals, put(base, corner, 100), (31, 7, 3, 3))
                case(f"tile_corner_freed/{cw}x{ch}/{fp_name}/{flags_name}", cw, ch, put(base, corner, 100), p, fp, goals, base, (31, 7, 3, 3))
    # a wall beside the goal cell: the rectangle fits along the wall only, so the goal keeps some headings and loses others;
    # and the way back: the headings the solve skipped become passable and still are no goals (rule c)
    open_ground = S.empty(w, h)
    walled = put(open_ground, [(x, 10) for x in range(20, 45)], 100)
    for flags_name, p in (("none", P_NONE), ("both", P_BOTH)):
        case(f"goal_headings_rejected/{flags_name}", w, h, open_ground, p, S.RECT_9x3, [(32, 8, -1)], walled, (20, 10, 25, 1), "raises")
        case(f"goal_heading_skipped_then_passable/{flags_name}", w, h, walled, p, S.RECT_9x3, [(32, 8, -1)], open_ground, (20, 10, 25, 1), "lowers")
    return out


def cases(w=None, h=None):
    """every case, or those of a shape"""
    if not _CASES:
        table = _named()
        for sw, sh in SHAPES:
            sets = [("point", S.POINT, P_NONE, "none"), ("point", S.POINT, P_BOTH, "both")]
            if sw >= 31 and sh >= 7:
                sets += [("9x3", S.RECT_9x3, P_BOTH, "both"), ("L", S.L_SHAPE, P_NONE, "none")]
            for fp_name, fp, p, flags_name in sets:
                table += _generic(sw, sh, fp_name, fp, p, flags_name)
        names = [c["name"] for c in table]
        assert len(set(names)) == len(names)
        _CASES["all"] = table
    return [c for c in _CASES["all"] if w is None or (c["w"], c["h"]) == (w, h)]


def given_plane(c, seed=99):
    """what the caller hands over: the new plane inside the window, garbage outside it (all of the new plane for None)"""
    if c["window"] is None:
        return c["new"].copy()
    out = garbage_plane(np.random.default_rng(seed), c["w"], c["h"])
    r = Q.clip(c["w"], c["h"], c["window"])
    if r is not None:
        xa, ya, xb, yb = r
        out[ya:yb, xa:xb] = c["new"][ya:yb, xa:xb]
    return out


def garbage_plane(rng, w, h):
    """any byte, half of the cells lethal"""
    plane = rng.integers(-128, 128, (h, w)).astype(np.int8)
    plane[rng.random((h, w)) < 0.5] = 100
    return plane


def references(c):
    """(the solve of the kept plane, the re-solve) of a case, once"""
    if c["name"] not in _REFS:
        first = R.solve(geo_of(c["w"], c["h"]), c["kept"], c["p"], c["fp"], c["goals"])
        assert not first["error"], c["name"]
        _REFS[c["name"]] = (first, Q.resolve(geo_of(c["w"], c["h"]), c["kept"], c["new"], c["window"], c["p"], c["fp"], first))
    return _REFS[c["name"]]
