"""The re-solve of the navigation field, the parts that need no GPU: the reference's raise-then-relax
(tests/navfield_resolve_ref.py) against navfield_ref.solve of the merged plane, in both forms, on 400 random cases; the
least raised set against the threshold set; two rooms and their door; the window-to-tile-range rule of
csrc/navfield_host.cpp under sanitizers; the declarations and the mirrors."""
import ctypes as C
import os
import random
import re

import numpy as np

from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_resolve_ref as RR
from tests import navfield_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_navfield_resolve", "lom_navfield_resolve_device", "lom_navfield_resolve_from_clearance",
               "lom_navfield_resolve_stats"]
P0 = N.params(50, 3, 400, 98)


def geo_of(w, h):
    return N.geometry(0.25, -3.0, 2.0, w, h)


def random_case(rng, w, h, p):
    """(kept plane, P of its solve, the plane given -- garbage outside the window --, the window, the merged plane wanted)"""
    nprng = np.random.default_rng(rng.randrange(1 << 30))
    kept = S.random_plane(nprng, w, h, obstacles=rng.choice([0.1, 0.3]), unknown=0.1)
    goals = np.array([(rng.randrange(w), rng.randrange(h)) for _ in range(rng.choice([1, 1, 3]))])
    first = N.solve(geo_of(w, h), kept, p, goals)
    ww, hh = rng.randrange(1, max(2, w // 2 + 1)), rng.randrange(1, max(2, h // 2 + 1))
    window = (rng.randrange(-2, w), rng.randrange(-2, h), ww, hh)
    want = kept.copy()
    given = S.random_plane(nprng, w, h)                               # garbage outside the window
    r = RR.clip(w, h, window)
    if r is not None:
        xa, ya, xb, yb = r
        want[ya:yb, xa:xb] = S.random_plane(nprng, xb - xa, yb - ya, obstacles=rng.choice([0.0, 0.3, 0.9]), unknown=0.1)
        given[ya:yb, xa:xb] = want[ya:yb, xa:xb]
    return kept, first["P"], given, window, want


def test_raise_then_relax_is_the_full_solve_on_400_random_cases():
    rng = random.Random(5)
    least_total = threshold_total = reached_total = 0
    for _ in range(400):
        w, h = rng.choice([(1, 1), (1, 20), (7, 5), (20, 13), (33, 17)])
        p = rng.choice([N.params(1, 0, 0, 98), N.params(50, 3, 200, 60, 1), N.params(N.MAX_CELL_COST, 0, 0, 98)])
        kept, P_old, given, window, want = random_case(rng, w, h, p)
        merged = RR.merged_plane(kept, given, window)
        assert np.array_equal(merged, want)
        full = N.solve(geo_of(w, h), merged, p, RR.derived_goals(P_old))
        least, n_least = RR.raise_then_relax(P_old, kept, merged, p, 0)
        thresh, n_thresh = RR.raise_then_relax(P_old, kept, merged, p, 1)
        assert least.tobytes() == full["P"].tobytes(), (w, h, window)
        assert thresh.tobytes() == full["P"].tobytes(), (w, h, window)
        assert n_least <= n_thresh, (w, h, window, n_least, n_thresh)   # the least set is never the larger
        ref = RR.resolve(geo_of(w, h), kept, given, window, p, P_old, with_threshold=True)
        assert (ref["cells_raised"], ref["cells_raised_threshold"]) == (n_least, n_thresh)
        assert ref["cells_changed"] == int((kept != merged).sum())
        s0 = N.solve(geo_of(w, h), kept, p, RR.derived_goals(P_old))["summary"]
        assert ref["summary"]["goals_used"] + ref["summary"]["goals_rejected"] == s0["goals_used"]
        least_total, threshold_total, reached_total = least_total + n_least, threshold_total + n_thresh, reached_total + int((P_old != RR.U).sum())
    assert 0 < least_total < threshold_total < reached_total


def test_the_least_set_of_an_unchanged_plane_is_empty():
    w, h = 33, 17
    plane = S.random_plane(np.random.default_rng(2), w, h)
    first = N.solve(geo_of(w, h), plane, P0, np.array([(3, 3), (30, 10)]))
    ref = RR.resolve(geo_of(w, h), plane, plane, None, P0, first["P"])
    assert ref["cells_changed"] == 0 and ref["cells_raised"] == 0 and ref["P"].tobytes() == first["P"].tobytes()


def test_two_rooms_and_their_door():
    w, h, door = 41, 23, 6
    geo = geo_of(w, h)
    open_plane = S.two_rooms(w, h, door)
    first = N.solve(geo, open_plane, P0, np.array([(3, 17)]))
    assert first["summary"]["cells_unreached"] == 0
    closed = open_plane.copy()
    closed[door, w // 2] = 100
    window = (w // 2, door, 1, 1)
    ref = RR.resolve(geo, open_plane, closed, window, P0, first["P"])
    far = np.zeros((h, w), bool)
    far[:, w // 2 + 1:] = True
    assert (ref["P"][far] == RR.U).all() and (ref["P"][:, :w // 2] != RR.U).all()
    P = RR.as_rows(first["P"])
    assert RR.drop_impassable(P, ref["costs"]) == 1                   # the door itself is the diff's
    rose = RR.least_raised_set(P, ref["costs"])
    assert rose == {(x, y) for y in range(h) for x in range(w // 2 + 1, w)} and ref["cells_raised"] == len(rose)
    # opening it again raises nothing: every kept value still has its supporter
    again = RR.resolve(geo, closed, open_plane, window, P0, ref["P"])
    assert again["cells_raised"] == 0 and again["cells_changed"] == 1
    assert again["P"].tobytes() == first["P"].tobytes()
    got, n = RR.raise_then_relax(ref["P"], closed, open_plane, P0, 0)
    assert n == 0 and got.tobytes() == first["P"].tobytes()


def test_tile_range_under_sanitizers(tmp_path):
    """tests/cpp/test_navfield_resolve.cpp compiles csrc/navfield_host.cpp and csrc/clearance_host.cpp alone: the clipped
    window's tiles at the grid's edges, at tile borders and for windows outside the grid"""
    exe = cpp_program.build_host(tmp_path, "test_navfield_resolve.cpp", ["navfield_host.cpp", "clearance_host.cpp"])
    cpp_program.run(exe, timeout=300)


def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"LOM_NAV_OPT_TEST_RESOLVE_FORM\s*=\s*4", text) and lom.capi.NAV_OPT_TEST_RESOLVE_FORM == 4
    assert re.search(r"Re-solve\.", text) and re.search(r"\} lom_navfield_resolve_counters;", text)
    assert C.sizeof(lom.capi.NavFieldResolveCounters) == 48
    assert [k for k, _ in lom.capi.NavFieldResolveCounters._fields_] == ["cells_changed", "cells_raised", "raise_launches",
                                                                         "relax_launches", "waits", "tiles_marked"]
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for name, method in (("resolve", "resolve"), ("resolveFromClearance", "resolveFromClearance"), ("resolveStats", "resolveStats")):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert hasattr(lom.NavField, method), method
    L = lom.capi.lib()
    st = lom.capi.NavFieldResolveCounters()
    assert L.lom_navfield_resolve(None, None, None, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_resolve_device(None, None, None, None, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_resolve_from_clearance(None, None, None, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_resolve_stats(None, C.byref(st)) == lom.capi.ERR_ARG
