"""The shift with a re-solve of the navigation field, the parts that need no GPU: the reference's incremental form (move,
drop, least raised set, relax; tests/navfield_shift_ref.py) against navfield_ref.solve of the merged plane on windows cut from
a larger world; the identity of the three goal counts; (0, 0) against navfield_resolve_ref.resolve; the declarations and the
mirrors."""
import ctypes as C
import os
import random
import re

import numpy as np

from tests import grid_shift_ref as GS
from tests import navfield_ref as N
from tests import navfield_resolve_ref as RR
from tests import navfield_scenes as S
from tests import navfield_shift_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_navfield_shift_resolve", "lom_navfield_shift_resolve_device", "lom_navfield_shift_resolve_from_clearance",
               "lom_navfield_shift_stats"]
SHAPES = [(1, 1), (1, 20), (7, 5), (20, 13), (33, 17), (65, 33)]


def geo_of(w, h):
    return N.geometry(0.25, -3.0, 2.0, w, h)


def world_case(rng, w, h):
    """a drive over a world: (kept window, P of its solve, params, dx, dy, new window -- with changes in `window` --, window)"""
    nprng = np.random.default_rng(rng.randrange(1 << 30))
    pad = 6
    world = S.random_plane(nprng, w + 2 * pad, h + 2 * pad, obstacles=rng.choice([0.05, 0.2, 0.4]), unknown=0.1)
    p = rng.choice([N.params(1, 0, 0, 98), N.params(50, 3, 200, 60, 1), N.params(N.MAX_CELL_COST, 0, 0, 98)])
    kept = SR.cut(world, pad, pad, w, h)
    goals = np.array([(rng.randrange(w), rng.randrange(h)) for _ in range(rng.choice([1, 2, 4]))])
    first = N.solve(geo_of(w, h), kept, p, goals)
    dx, dy = rng.randrange(-5, 6), rng.randrange(-5, 6)
    new = SR.cut(world, pad + dx, pad + dy, w, h).copy()
    window = rng.choice([None, (0, 0, 0, 0), (rng.randrange(-2, w), rng.randrange(-2, h), rng.randrange(1, w + 2), rng.randrange(1, h + 2))])
    r = RR.clip(w, h, window)
    if r is not None and window is not None:                            # cells change inside the kept overlap as well
        xa, ya, xb, yb = r
        new[ya:yb, xa:xb] = S.random_plane(nprng, xb - xa, yb - ya, obstacles=rng.choice([0.0, 0.3, 0.9]), unknown=0.1)
    return kept, first, p, dx, dy, new, window, nprng


def test_the_incremental_form_is_the_full_solve_on_windows_of_a_world():
    rng = random.Random(11)
    raised = reached = left = rejected = 0
    for k in range(204):
        w, h = SHAPES[k % len(SHAPES)]
        kept, first, p, dx, dy, new, window, nprng = world_case(rng, w, h)
        ref = SR.shift_resolve(geo_of(w, h), kept, new, window, p, first["P"], dx, dy)
        assert ref["status"] == GS.OK
        given = SR.given_plane(new, ref["taken"], nprng)                 # garbage where the plane is not read
        P_moved, moved, mask = SR.moved_state(first["P"], kept, dx, dy)
        merged, _ = SR.merged_plane(moved, mask, given, window)
        assert np.array_equal(merged, ref["plane"])
        if window is None:
            assert np.array_equal(merged, new)                           # the whole grid: the window of the world at its new place
        got, n = SR.incremental(P_moved, merged, p)
        assert got.tobytes() == ref["P"].tobytes(), (k, w, h, dx, dy, window)
        assert n == ref["cells_raised"]
        # the goals: what the last solve used is used, rejected or has left
        s = ref["summary"]
        assert first["summary"]["goals_used"] == s["goals_used"] + s["goals_rejected"] + ref["goals_left"], (k, dx, dy)
        assert ref["cells_kept"] + ref["cells_entered"] == w * h
        assert ref["cells_kept"] == max(0, w - abs(dx)) * max(0, h - abs(dy))
        raised, reached = raised + n, reached + s["cells_reached"]
        left, rejected = left + ref["goals_left"], rejected + s["goals_rejected"]
    assert raised > 0 and reached > 0 and left > 0 and rejected > 0      # (the cases cover all four)


def test_a_zero_shift_is_the_resolve():
    rng = random.Random(3)
    for k in range(20):
        w, h = SHAPES[2 + k % 3]
        kept, first, p, _, _, new, window, _ = world_case(rng, w, h)
        ref = SR.shift_resolve(geo_of(w, h), kept, new, window, p, first["P"], 0, 0)
        want = RR.resolve(geo_of(w, h), kept, new, window, p, first["P"])
        assert ref["P"].tobytes() == want["P"].tobytes() and ref["summary"] == want["summary"]
        assert np.array_equal(ref["plane"], want["plane"])
        assert (ref["cells_changed"], ref["cells_raised"]) == (want["cells_changed"], want["cells_raised"])
        assert (ref["cells_kept"], ref["cells_entered"], ref["goals_left"]) == (w * h, 0, 0)
        assert GS.geometry_bits(ref["geo"]) == GS.geometry_bits(geo_of(w, h))


def test_what_the_scenes_are_for():
    """a trailing border whose supporters left rises; a border whose supporters lie towards the goal does not"""
    w, h = 41, 23
    geo, p = geo_of(w, h), N.params(50, 3, 400, 98)
    # a U on its side, open to the right: the bend at x = 1 leaves with a shift of 3, the far arm rises and stays unreached
    u = np.full((h, w), 100, np.int8)
    u[5, 1:], u[15, 1:], u[5:16, 1] = 0, 0, 0
    first = N.solve(geo, u, p, np.array([(w - 1, 5)]))
    assert first["summary"]["cells_reached"] == 2 * (w - 1) + 9
    ref = SR.shift_resolve(geo, u, SR.cut(u, 3, 0, w, h), None, p, first["P"], 3, 0)
    assert ref["cells_raised"] == w - 3 and ref["summary"]["cells_reached"] == w - 3 and ref["goals_left"] == 0
    assert (ref["P"][15] == SR.U).all() and ref["summary"]["cells_unreached"] == w - 3
    # free ground, the goal in the middle: every border cell's supporter lies towards the goal
    e = S.empty(w, h)
    first = N.solve(geo, e, p, np.array([(w // 2, h // 2)]))
    ref = SR.shift_resolve(geo, e, e, None, p, first["P"], 1, 0)
    assert ref["cells_raised"] == 0 and ref["cells_entered"] == h and ref["summary"]["cells_unreached"] == 0
    # a shift that keeps nothing: no goals, every cell unreached
    ref = SR.shift_resolve(geo, e, e, None, p, first["P"], w, 0)
    assert ref["goals_left"] == 1 and ref["summary"]["cells_reached"] == 0 and ref["summary"]["goals_used"] == 0
    # the rule's refusal
    big = dict(resolution=1e30, origin_x=3e38, origin_y=0.0, width=w, height=h)
    assert SR.shift_resolve(big, e, e, None, p, first["P"], GS.I32_MAX, 0)["status"] == GS.ERR_RANGE


def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"Shift and re-solve\.", text) and re.search(r"\} lom_navfield_shift_counters;", text)
    assert re.search(r"#define LOM_ABI_VERSION 2\b", text)               # the change only adds
    assert C.sizeof(lom.capi.NavFieldShiftCounters) == 24 and C.sizeof(lom.capi.NavFieldResolveCounters) == 48
    assert [k for k, _ in lom.capi.NavFieldShiftCounters._fields_] == ["cells_kept", "cells_entered", "goals_left"]
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for method in ("shiftResolve", "shiftResolveFromClearance", "shiftStats"):
        assert re.search(r"\b%s\s*\(" % method, mirror), method
        assert hasattr(lom.NavField, method), method
    L = lom.capi.lib()
    st, sm = lom.capi.NavFieldShiftCounters(), lom.capi.NavFieldSummary()
    sm.cells_blocked = 9
    assert L.lom_navfield_shift_resolve(None, 1, 1, None, None, C.byref(sm)) == lom.capi.ERR_ARG and sm.cells_blocked == 0
    assert L.lom_navfield_shift_resolve_device(None, 1, 1, None, None, None, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_shift_resolve_from_clearance(None, 1, 1, None, None, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_shift_stats(None, C.byref(st)) == lom.capi.ERR_ARG
