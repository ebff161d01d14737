"""The shift with a re-solve of the navigation field on the device against tests/navfield_shift_ref.py: windows are cut from a
larger world, a field is solved on one, and lom_navfield_shift_resolve* moves it to the next.  Bytes are compared, with no
tolerance anywhere: the field, the summary, cells_changed and (under the default form) cells_raised, the three counts of
lom_navfield_shift_stats, the geometry's bits, and paths, queries, waypoints and visibility on the new state.  Every case hands
over garbage where the new plane is not read.  The references of a case are computed once and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import grid_shift_ref as GS
from tests import navfield_ref as N
from tests import navfield_resolve_ref as RR
from tests import navfield_scenes as S
from tests import navfield_shift_ref as SR
from tests import navfield_waypoints_ref as W

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)                       # dyadic: every origin on the way is exact
P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 31), (65, 33), (129, 65)]   # the tile is 32 x 32: the last three have tile borders and a corner
CROSSED = [(33, 31), (65, 33)]                        # every pair of shifts; a seeded sample of about twenty elsewhere
SCENES = ("sparse", "dense", "serpentine", "spiral", "two_rooms")
WINDOWS = ("whole", "empty", "patch", "edge")
SWITCHES = [(form, cap, every) for form in (0, 1, 2) for cap in (1, 0) for every in (0, 1)]
ZERO_STATS = dict(cells_changed=0, cells_raised=0, raise_launches=0, relax_launches=0, waits=0, tiles_marked=0)
REFS = {}


def geo_of(w, h, origin=ORIGIN):
    return N.geometry(RES, origin[0], origin[1], w, h)


def as_tuple(p):
    return (p["neutral"], p["factor"], p["unknown_cost"], p["max_passable"], p["flags"])


def axis_values(n):
    v = {0}
    for k in (1, 31, 32, 33, n - 1, n, n + 1):
        v |= {k, -k}
    return sorted(v)


def pairs_of(w, h):
    xs, ys = axis_values(w), axis_values(h)
    cross = [(dx, dy) for dx in xs for dy in ys]
    if (w, h) in CROSSED:
        return cross
    rng = np.random.default_rng(w * 10007 + h)
    fixed = list(dict.fromkeys([(0, 0), (1, 0), (0, -1), (-1, 1), (w, 0), (0, -h), (w - 1, h - 1)]))
    rest = [q for q in cross if q not in fixed]
    return fixed + [rest[i] for i in rng.choice(len(rest), min(len(rest), 21 - len(fixed)), replace=False)]


def set_switches(lom, dev, form, cap, every, batch=0):
    dev.setOption(lom.capi.NAV_OPT_TEST_RESOLVE_FORM, form)
    dev.setOption(lom.capi.NAV_OPT_TEST_INNER_CAP, cap)
    dev.setOption(lom.capi.NAV_OPT_TEST_ALL_TILES, every)
    dev.setOption(lom.capi.NAV_OPT_TEST_BATCH, batch)


def first_passable(plane, p, n):
    """n passable cells spread over the grid, the first one first, as goals (fewer where there are fewer)"""
    t = np.array(N.cell_costs(p))
    cells = np.argwhere(t[plane.view(np.uint8)] != 0)[:, ::-1].astype(np.int32).reshape(-1, 2)
    return cells[np.unique(np.linspace(0, len(cells) - 1, n).astype(int))] if len(cells) else cells


def world_of(scene, w, h):
    """(world plane, the window's place in it): room for a shift of n + 1 cells either way"""
    key = ("world", scene, w, h)
    if key not in REFS:
        ww, wh = 3 * w + 4, 3 * h + 4
        rng = np.random.default_rng(100 * w + h + len(scene))
        REFS[key] = dict(sparse=lambda: S.random_plane(rng, ww, wh, obstacles=0.05), dense=lambda: S.random_plane(rng, ww, wh, obstacles=0.3),
                         serpentine=lambda: S.serpentine(ww, wh), spiral=lambda: S.spiral(ww, wh),
                         two_rooms=lambda: S.two_rooms(ww, wh, wh // 2))[scene]()
    return REFS[key], (w + 2, h + 2)


def first_of(scene, w, h):
    """(kept plane, params, goals, the reference's solve) of the window before the shift, once"""
    key = ("first", scene, w, h)
    if key not in REFS:
        world, (ox, oy) = world_of(scene, w, h)
        kept = np.ascontiguousarray(SR.cut(world, ox, oy, w, h))
        p = P1 if scene in ("sparse", "dense") else P0
        goals = first_passable(kept, p, 3)
        REFS[key] = (kept, p, goals, N.solve(geo_of(w, h), kept, p, goals))
    return REFS[key]


def window_of(kind, w, h):
    return dict(whole=None, empty=(3, 3, 0, 9), patch=(w // 4, h // 4, max(w // 2, 1), max(h // 2, 1)), edge=(-2, h - 3, 6, 9))[kind]


def case_of(scene, w, h, dx, dy, kind):
    """(kept, params, goals, first, window, the plane given, the reference) of a case, once: the new plane is the world's window
    at its new place, with other cells inside a window that is not the whole grid (cells change inside the kept box)"""
    key = ("case", scene, w, h, dx, dy, kind)
    if key not in REFS:
        kept, p, goals, first = first_of(scene, w, h)
        world, (ox, oy) = world_of(scene, w, h)
        rng = np.random.default_rng([SCENES.index(scene), w, h, dx % (1 << 32), dy % (1 << 32), WINDOWS.index(kind)])
        new = np.ascontiguousarray(SR.cut(world, ox + dx, oy + dy, w, h)).copy()
        window = window_of(kind, w, h)
        r = RR.clip(w, h, window)
        if r is not None and window is not None:
            xa, ya, xb, yb = r
            new[ya:yb, xa:xb] = S.random_plane(rng, xb - xa, yb - ya, obstacles=0.2)
        ref = SR.shift_resolve(geo_of(w, h), kept, new, window, p, first["P"], dx, dy)
        REFS[key] = (kept, p, goals, first, window, SR.given_plane(new, ref["taken"], rng), ref)
    return REFS[key]


def expected_stats(ref):
    return dict(cells_kept=ref["cells_kept"], cells_entered=ref["cells_entered"], goals_left=ref["goals_left"])


def check_state(dev, ref, geo, summary, form, what):
    """what a shift with a re-solve left on the handle against the reference; returns lom_navfield_resolve_stats"""
    got, st = dev.potential(), dev.resolveStats()
    assert got.tobytes() == ref["P"].tobytes(), (what, np.argwhere(got != ref["P"])[:10])
    assert summary == ref["summary"], (what, summary, ref["summary"])
    assert st["cells_changed"] == ref["cells_changed"], (what, st, ref["cells_changed"])
    if form == 0:
        assert st["cells_raised"] == ref["cells_raised"], (what, st, ref["cells_raised"])
    assert dev.shiftStats() == expected_stats(ref), (what, dev.shiftStats(), expected_stats(ref))
    assert GS.geometry_bits(dev.geometry()) == GS.geometry_bits(geo), (what, dev.geometry(), geo)
    return st


def check_reads(dev, ref, geo, rng, what):
    """paths, the query, waypoints and visibility read the new state, in the new geometry"""
    w, h = geo["width"], geo["height"]
    ox, oy = float(geo["origin_x"]), float(geo["origin_y"])
    starts = np.concatenate([np.stack([rng.integers(0, w, 6), rng.integers(0, h, 6)], axis=1),
                             np.array([(0, 0), (w - 1, h - 1), (-1, 0), (w, h - 1)])]).astype(np.int32)
    cells, lengths = dev.paths(starts, 40)
    want_cells, want_lengths = N.paths(geo, ref["costs"], ref["P"], starts, 40)
    assert np.array_equal(lengths, want_lengths) and cells.tobytes() == want_cells.tobytes(), what
    xy = np.concatenate([rng.uniform(ox - 1.0, ox + w * RES + 1.0, (40, 1)), rng.uniform(oy - 1.0, oy + h * RES + 1.0, (40, 1))],
                        axis=1).astype(np.float32)
    assert np.array_equal(dev.query(xy), N.query(geo, ref["P"], xy)), what
    want = W.waypoints(geo, ref["costs"], ref["P"], starts, 0, 16, 200, 12)
    got = dev.waypoints(starts, (0, 16, 200, 0), 12)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), what
    pairs = np.concatenate([starts[:-1], starts[1:]], axis=1).astype(np.int32)
    assert np.array_equal(dev.visible(pairs), W.visible_many(ref["costs"], w, h, pairs)), what


def run_case(lom, dev, geo, scene, w, h, dx, dy, kind, form, cap, every, reads=None, batch=0):
    """solve the window before the shift on `dev` (whose geometry is `geo`), shift and re-solve, compare; returns the new geometry"""
    kept, p, goals, first, window, given, ref = case_of(scene, w, h, dx, dy, kind)
    assert ref["status"] == GS.OK
    set_switches(lom, dev, form, 0, 0)
    assert dev.solve(kept, as_tuple(p), goals) == first["summary"]
    set_switches(lom, dev, form, cap, every, batch)
    status, moved = GS.shift_geometry(geo, dx, dy)
    assert status == GS.OK
    what = (scene, w, h, dx, dy, kind, form, cap, every)
    check_state(dev, ref, moved, dev.shiftResolve(dx, dy, given, window), form, what)
    if reads is not None:
        check_reads(dev, ref, moved, reads, what)
    return moved


# ---- 1: shapes x shifts, with scenes, windows and switches taken in turn ---------------------------------------------------------
def shift_params():
    out = []
    for w, h in SHAPES:
        if (w, h) in CROSSED:
            out += [pytest.param(w, h, dx, id=f"{w}x{h}-dx{dx}") for dx in axis_values(w)]
        else:
            out.append(pytest.param(w, h, None, id=f"{w}x{h}"))
    return out


@pytest.mark.parametrize("w,h,only_dx", shift_params())
def test_shapes_and_shifts(lom, w, h, only_dx):
    rng = np.random.default_rng(w + 7 * h)
    dev, geo = lom.NavField(RES, ORIGIN, w, h), geo_of(w, h)
    pairs = [q for q in pairs_of(w, h) if only_dx is None or q[0] == only_dx]
    assert len(pairs) >= (11 if only_dx is not None else 1)
    for k, (dx, dy) in enumerate(pairs):
        n = k + abs(dx) + 3 * abs(dy)
        form, cap, every = SWITCHES[n % len(SWITCHES)]
        geo = run_case(lom, dev, geo, SCENES[n % len(SCENES)], w, h, dx, dy, WINDOWS[(n // 5) % len(WINDOWS)], form, cap, every,
                       reads=rng if k % 6 == 0 else None)


@pytest.mark.parametrize("w,h", SHAPES[3:])
def test_the_switch_cross_on_the_bordered_shapes(lom, w, h):
    """forms 0 / 1 / 2 x inner cap 1 / default x all tiles on / off: the same bytes, and under the default form the
    reference's cells_raised whatever the schedule"""
    dev, geo = lom.NavField(RES, ORIGIN, w, h), geo_of(w, h)
    for scene, dx, dy, kind in (("dense", 1, 0, "patch"), ("serpentine", -33, 2, "whole"), ("two_rooms", 0, 0, "patch"),
                                ("sparse", w - 1, -(h - 1), "edge"), ("spiral", 3, -31 if h > 31 else -30, "empty")):
        for form, cap, every in SWITCHES:
            for batch in ((1, 8, 0) if (w, h) == (65, 33) and scene == "dense" else (0,)):
                geo = run_case(lom, dev, geo, scene, w, h, dx, dy, kind, form, cap, every, batch=batch)


def test_shifts_beyond_every_side(lom):
    """INT32_MAX and INT32_MIN keep nothing where the geometry rule takes them, and are its refusal where it does not"""
    w, h = 33, 31
    kept, p, goals, first = first_of("sparse", w, h)
    new = S.random_plane(np.random.default_rng(5), w, h, obstacles=0.1)
    for dx, dy in ((GS.I32_MAX, 0), (0, GS.I32_MIN), (GS.I32_MIN, GS.I32_MAX), (GS.I32_MAX, 1)):
        dev = lom.NavField(RES, ORIGIN, w, h)
        assert dev.solve(kept, as_tuple(p), goals) == first["summary"]
        ref = SR.shift_resolve(geo_of(w, h), kept, new, (0, 0, 0, 0), p, first["P"], dx, dy)
        assert ref["status"] == GS.OK and ref["cells_kept"] == 0 and ref["goals_left"] == first["summary"]["goals_used"]
        assert ref["summary"]["cells_reached"] == 0 and np.array_equal(ref["plane"], new)
        check_state(dev, ref, ref["geo"], dev.shiftResolve(dx, dy, new, (0, 0, 0, 0)), 0, (dx, dy))
        assert dev.resolve(new) == ref["summary"]                       # the field is solved: a re-solve is taken
    # an origin that the rule cannot move: the range refusal, and nothing changes
    dev = lom.NavField(1e30, (3e38, 0.0), w, h)
    assert dev.solve(kept, as_tuple(p), goals) == first["summary"]
    before, geo = dev.potential(), dev.geometry()
    assert GS.shift_geometry(geo, GS.I32_MAX, 0)[0] == GS.ERR_RANGE
    with pytest.raises(lom.LomError) as e:
        dev.shiftResolve(GS.I32_MAX, 0, new)
    assert e.value.code == lom.capi.ERR_RANGE and dev.potential().tobytes() == before.tobytes()
    assert GS.geometry_bits(dev.geometry()) == GS.geometry_bits(geo)
    assert dev.resolve(kept)["goals_used"] == first["summary"]["goals_used"]


# ---- 2: scenes arranged for what a shift does to a field -------------------------------------------------------------------------
def arranged(w, h):
    """name -> (kept plane, goals, dx, dy, new plane, window, what the reference must show)"""
    free = S.empty(w, h)
    u = np.full((h, w), 100, np.int8)                                   # a U on its side, open to the right, its bend at x = 1
    u[5, 1:], u[25, 1:], u[5:26, 1] = 0, 0, 0
    rooms = S.two_rooms(w, h, 0)                                        # the door in row 0
    rooms_up = np.ascontiguousarray(GS.shift_array(rooms, 0, 1, 0))
    rooms_up[:, w // 2] = 100                                           # the wall goes on, with no door
    patch = S.random_plane(np.random.default_rng(8), w, h, obstacles=0.25)
    two = np.array([(1, 5), (60, 20)], np.int32)
    return {
        "a_goal_leaves_another_stays": (free, two, 4, 0, free, None,
                                        lambda r: r["goals_left"] == 1 and r["summary"]["goals_used"] == 1 and r["cells_raised"] > 100),
        "all_goals_leave": (free, two, 0, 25, free, None,
                            lambda r: r["goals_left"] == 2 and r["summary"]["cells_reached"] == 0 and r["cells_raised"] == w * (h - 25)),
        "the_bend_of_a_u_leaves": (u, np.array([(w - 1, 5)], np.int32), 3, 0, SR.cut(u, 3, 0, w, h), None,
                                   lambda r: r["cells_raised"] == w - 3 and (r["P"][25] == SR.U).all() and r["summary"]["cells_reached"] == w - 3),
        "a_door_leaves": (rooms, np.array([(3, 17)], np.int32), 0, 1, rooms_up, None,
                          lambda r: r["cells_raised"] == (w - w // 2 - 1) * (h - 1) and (r["P"][:, w // 2 + 1:] == SR.U).all()),
        "a_kept_goal_becomes_impassable": (free, np.array([(30, 10), (50, 20)], np.int32), 2, 3, np.full((h, w), 100, np.int8), (28, 7, 1, 1),
                                           lambda r: r["summary"]["goals_rejected"] == 1 and r["summary"]["goals_used"] == 1 and r["cells_changed"] == 1),
        "cells_change_inside_the_kept_box": (free, two, -2, 1, patch, (10, 5, 40, 20),
                                             lambda r: r["cells_changed"] > 150 and r["goals_left"] == 0 and r["cells_entered"] == 2 * h + w - 2),
    }


def test_arranged_scenes(lom):
    w, h = 65, 33
    rng = np.random.default_rng(2)
    for name, (kept, goals, dx, dy, new, window, shows) in arranged(w, h).items():
        first = N.solve(geo_of(w, h), kept, P0, goals)
        ref = SR.shift_resolve(geo_of(w, h), kept, new, window, P0, first["P"], dx, dy)
        assert shows(ref), (name, {k: ref[k] for k in ("cells_changed", "cells_raised", "cells_entered", "goals_left", "summary")})
        given = SR.given_plane(np.ascontiguousarray(new), ref["taken"], rng)
        for form, cap, every in ((0, 0, 0), (0, 1, 1), (1, 0, 0), (2, 1, 0)):
            dev = lom.NavField(RES, ORIGIN, w, h)
            set_switches(lom, dev, form, cap, every)
            assert dev.solve(kept, as_tuple(P0), goals) == first["summary"]
            check_state(dev, ref, ref["geo"], dev.shiftResolve(dx, dy, given, window), form, (name, form, cap, every))
        check_reads(dev, ref, ref["geo"], rng, name)


def test_a_border_whose_supporters_lie_towards_the_goal_does_not_rise(lom):
    """an empty 129 x 65 plane, one goal at (64, 32), a shift of (1, 0), one sweep per launch: nothing rises, and the raise and
    relax launches together are strictly fewer than those of the full relaxation from the goal on the same handle"""
    w, h = 129, 65
    kept, goals = S.empty(w, h), np.array([(64, 32)], np.int32)
    first = N.solve(geo_of(w, h), kept, P0, goals)
    ref = SR.shift_resolve(geo_of(w, h), kept, kept, None, P0, first["P"], 1, 0)
    assert ref["cells_raised"] == 0 and ref["cells_entered"] == h and ref["summary"]["cells_unreached"] == 0
    dev, stats = lom.NavField(RES, ORIGIN, w, h), {}
    for form in (0, 2):
        set_switches(lom, dev, form, 1, 0, batch=1)                     # a wait per launch: the counts are exact
        dev.shift(-1, 0) if form == 2 else None                         # (back to the first origin)
        assert dev.solve(kept, as_tuple(P0), goals) == first["summary"]
        stats[form] = check_state(dev, ref, ref["geo"], dev.shiftResolve(1, 0, kept), form, form)
    assert stats[0]["cells_raised"] == 0 and stats[0]["raise_launches"] >= 1
    assert stats[0]["raise_launches"] + stats[0]["relax_launches"] < stats[2]["raise_launches"] + stats[2]["relax_launches"], stats


# ---- 3: (0, 0), sequences, out and back --------------------------------------------------------------------------------------------
def test_a_zero_shift_is_the_resolve_on_a_twin_handle(lom):
    w, h = 65, 33
    rng = np.random.default_rng(19)
    kept, new = S.random_plane(rng, w, h, obstacles=0.2), S.random_plane(rng, w, h, obstacles=0.3)
    goals = first_passable(kept, P1, 3)
    for form in (0, 1, 2):
        for window in (None, (20, 10, 30, 15), (3, 3, 0, 9), (w, 0, 5, 5)):
            a, b = lom.NavField(RES, ORIGIN, w, h), lom.NavField(RES, ORIGIN, w, h)
            for dev in (a, b):
                set_switches(lom, dev, form, 0, 0)
                dev.solve(kept, as_tuple(P1), goals)
            assert a.shiftResolve(0, 0, new, window) == b.resolve(new, window), (form, window)
            assert a.potential().tobytes() == b.potential().tobytes() and a.resolveStats() == b.resolveStats(), (form, window)
            assert a.shiftStats() == dict(cells_kept=w * h, cells_entered=0, goals_left=0)
            assert GS.geometry_bits(a.geometry()) == GS.geometry_bits(b.geometry())
            ref = SR.shift_resolve(geo_of(w, h), kept, new, window, P1, N.solve(geo_of(w, h), kept, P1, goals)["P"], 0, 0)
            assert a.potential().tobytes() == ref["P"].tobytes()


DRIVE = [(3, 0), (2, 1), (0, 0), (1, -1), (32, 0), (-5, 4), (0, -7), (-33, 2), (1, 1), (4, 0), (0, 3), (-2, -2)]


def run_drive(lom, w, h):
    """twelve (shift, re-solve) steps through a world on one handle, each against the full model of the state so far"""
    world = S.random_plane(np.random.default_rng(31), w + 80, h + 40, obstacles=0.15)
    ox, oy = 40, 20
    geo = geo_of(w, h)
    kept = np.ascontiguousarray(SR.cut(world, ox, oy, w, h))
    goals = first_passable(kept, P1, 4)
    first = N.solve(geo, kept, P1, goals)
    dev = lom.NavField(RES, ORIGIN, w, h)
    assert dev.solve(kept, as_tuple(P1), goals) == first["summary"]
    P_old, out, rng = first["P"], [], np.random.default_rng(6)
    for k, (dx, dy) in enumerate(DRIVE):
        ox, oy = ox + dx, oy + dy
        new = np.ascontiguousarray(SR.cut(world, ox, oy, w, h))
        window = (None, (0, 0, 0, 0), (w // 3, h // 3, 20, 10))[k % 3]
        key = ("drive", w, h, k)
        if key not in REFS:
            REFS[key] = SR.shift_resolve(geo, kept, new, window, P1, P_old, dx, dy)
        ref = REFS[key]
        if k % 4 == 3:
            set_switches(lom, dev, 0, 1, k % 8 == 7)
        check_state(dev, ref, ref["geo"], dev.shiftResolve(dx, dy, SR.given_plane(new, ref["taken"], rng), window), 0, (k, dx, dy))
        geo, kept, P_old = ref["geo"], ref["plane"], ref["P"]
        out.append(dev.potential().tobytes())
    check_reads(dev, ref, geo, rng, "drive")
    assert ref["summary"]["cells_reached"] + ref["summary"]["cells_unreached"] > 0
    return out


def test_a_drive_of_twelve_steps_twice(lom):
    assert run_drive(lom, 65, 33) == run_drive(lom, 65, 33)


def test_out_and_back(lom):
    """what never left the grid and still has its route keeps its value; the whole equals the model both ways"""
    w, h = 65, 33
    kept = S.random_plane(np.random.default_rng(3), w, h, obstacles=0.1)
    goals = np.array([(32, 16)], np.int32)
    geo = geo_of(w, h)
    first = N.solve(geo, kept, P0, goals)
    dev = lom.NavField(RES, ORIGIN, w, h)
    assert dev.solve(kept, as_tuple(P0), goals) == first["summary"]
    out = SR.shift_resolve(geo, kept, SR.cut(kept, 5, -3, w, h, fill=0), None, P0, first["P"], 5, -3)
    check_state(dev, out, out["geo"], dev.shiftResolve(5, -3, out["plane"]), 0, "out")
    back = SR.shift_resolve(out["geo"], out["plane"], SR.cut(out["plane"], -5, 3, w, h, fill=0), None, P0, out["P"], -5, 3)
    check_state(dev, back, back["geo"], dev.shiftResolve(-5, 3, back["plane"]), 0, "back")
    assert GS.geometry_bits(dev.geometry()) == GS.geometry_bits(geo)
    never_left = GS.kept_mask(w, h, 5, -3) & GS.shift_array(GS.kept_mask(w, h, 5, -3), -5, 3, False)
    assert np.array_equal(back["plane"][never_left], kept[never_left]) and back["goals_left"] == 0


# ---- 4: the three forms of the call, the chain, refusals ---------------------------------------------------------------------------
def test_host_device_and_clearance_forms_leave_the_same_bytes(lom):
    import torch

    w, h = 129, 65
    rng = np.random.default_rng(23)
    cgeo = K.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)
    cp = K.params(1.0, 0.3, 1.5)
    table = lom.clearanceCostTable(cp, RES)
    occ_world = np.where(rng.random((h + 20, w + 20)) < 0.03, 100, 0).astype(np.int8)
    dx, dy = 7, -4
    occ0 = np.ascontiguousarray(SR.cut(occ_world, 10, 10, w, h, fill=0))
    occ1 = np.ascontiguousarray(SR.cut(occ_world, 10 + dx, 10 + dy, w, h, fill=0))
    clear = lom.ClearanceGrid(RES, ORIGIN, w, h)
    clear.update(occ0, None, cp)
    cost0 = K.update(cgeo, occ0, None, cp, None, K.empty_state(cgeo), table)["cost"]
    goals = first_passable(cost0, P0, 3)
    first = N.solve(geo_of(w, h), cost0, P0, goals)
    devs = [lom.NavField(RES, ORIGIN, w, h) for _ in range(3)]
    for dev in devs:
        assert dev.solveFromClearance(clear, as_tuple(P0), goals) == first["summary"]
    # the clearance grid follows and is updated in full: its shift is its clear
    clear.shift(dx, dy)
    clear.update(occ1, None, cp)
    cost1 = clear.cost()[0]
    status, moved = GS.shift_geometry(geo_of(w, h), dx, dy)
    assert np.array_equal(cost1, K.update(dict(cgeo, origin_x=float(moved["origin_x"]), origin_y=float(moved["origin_y"])), occ1, None, cp, None,
                                          K.empty_state(cgeo), table)["cost"])
    ref = SR.shift_resolve(geo_of(w, h), cost0, cost1, None, P0, first["P"], dx, dy)
    assert ref["cells_changed"] > 0 and ref["summary"]["cells_reached"] > 1000
    host, device, from_clear = devs
    check_state(host, ref, moved, host.shiftResolve(dx, dy, cost1), 0, "host")
    # a plane produced on another stream, at an odd byte offset: the call waits for the caller's event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.ones(1 << 24, device="cuda:0")
        for _ in range(10):                                              # work in front of the plane
            big = big * 1.0001 + 1.0
        block = torch.zeros(w * h + 3, dtype=torch.int8, device="cuda:0")
        block[3:] = torch.from_numpy(cost1.reshape(-1)).to("cuda:0", non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s)
    old = C.c_void_p()
    assert lom.capi.lib().lom_navfield_potential_device(device.handle, C.byref(old)) == 0
    summary = device.shiftResolve(dx, dy, block.data_ptr() + 3, None, device=True, hip_event=C.c_void_p(ev.cuda_event))
    check_state(device, ref, moved, summary, 0, "device")
    now = C.c_void_p()
    assert lom.capi.lib().lom_navfield_potential_device(device.handle, C.byref(now)) == 0 and now.value != old.value   # the second block
    block.fill_(100)
    torch.cuda.synchronize()
    check_reads(device, ref, moved, rng, "device")                      # the field keeps its own copy of the plane
    # a clearance grid that was not shifted is refused, and nothing changes
    unshifted = lom.ClearanceGrid(RES, ORIGIN, w, h)
    unshifted.update(occ1, None, cp)
    before, stats = from_clear.potential(), (from_clear.resolveStats(), from_clear.shiftStats())
    with pytest.raises(lom.LomError) as e:
        from_clear.shiftResolveFromClearance(dx, dy, unshifted)
    assert e.value.code == lom.capi.ERR_ARG and "resolution, origin, width or height differs" in str(e.value)
    assert from_clear.potential().tobytes() == before.tobytes() and (from_clear.resolveStats(), from_clear.shiftStats()) == stats
    assert GS.geometry_bits(from_clear.geometry()) == GS.geometry_bits(geo_of(w, h))
    check_state(from_clear, ref, moved, from_clear.shiftResolveFromClearance(dx, dy, clear), 0, "from the clearance grid")
    assert host.potential().tobytes() == device.potential().tobytes() == from_clear.potential().tobytes()
    torch.cuda.synchronize()


def test_the_chain_follows_and_keeps_its_field(lom):
    """occupancy + elevation shifted, clearance shifted and updated from the grids, the field shifted and re-solved from the
    clearance grid, the rollouts over both: equal to the references' chain"""
    from tests import rollout_ref as RO
    from tests import test_grid_shift_gpu as G
    from tests.rollout_scenes import commands_of, states_of

    geo = K.geometry(G.RES, G.C_ORG[0], G.C_ORG[1], G.CW, G.CH)
    c = dict(occ=lom.OccupancyGrid(G.RES, G.C_ORG, G.CW, G.CH), elev=lom.ElevationGrid(G.RES, G.C_ORG, G.CW, G.CH, G.Z_REF),
             clear=lom.ClearanceGrid(G.RES, G.C_ORG, G.CW, G.CH), nav=lom.NavField(G.RES, G.C_ORG, G.CW, G.CH),
             roll=lom.RolloutGrid(G.RES, G.C_ORG, G.CW, G.CH))
    table = lom.clearanceCostTable(G.C_CP, G.RES)
    for scan, pose in zip(G.chain_scans(), G.C_POSES):
        c["occ"].integrateCloud(scan, pose, G.C_RAY)
        c["elev"].integrateCloud(scan, pose, G.C_PNT)
    c["clear"].updateFromGrids(c["occ"], G.RULE, c["elev"], G.C_LAYER, G.C_COST, G.C_CP)
    got = c["nav"].solveFromClearance(c["clear"], G.C_NP, G.C_GOALS)
    cost0, pot0 = c["clear"].cost()[0], c["nav"].potential()
    ref = N.solve(geo, cost0, N.params(*G.C_NP), G.C_GOALS)
    assert got == ref["summary"] and pot0.tobytes() == ref["P"].tobytes()
    dx, dy = 7, -4
    for name in ("occ", "elev", "clear", "roll"):
        c[name].shift(dx, dy)
    status, moved = GS.shift_geometry(geo, dx, dy)
    moved = dict(moved, origin_x=float(moved["origin_x"]), origin_y=float(moved["origin_y"]))
    got_clear = c["clear"].updateFromGrids(c["occ"], G.RULE, c["elev"], G.C_LAYER, G.C_COST, G.C_CP)
    got_nav = c["nav"].shiftResolveFromClearance(dx, dy, c["clear"])
    occ, elev, cost = c["occ"].classify(G.RULE)[0], c["elev"].cost(G.C_LAYER, G.C_COST)[0], c["clear"].cost()[0]
    want = K.update(moved, occ, elev, G.C_CP, None, K.empty_state(moved), table)
    assert not want["error"] and got_clear == want["summary"] and np.array_equal(cost, want["cost"])
    ref = SR.shift_resolve(geo, cost0, cost, None, N.params(*G.C_NP), pot0, dx, dy)
    check_state(c["nav"], ref, moved, got_nav, 0, "chain")
    assert ref["summary"]["cells_reached"] > 500 and ref["cells_kept"] == (G.CW - 7) * (G.CH - 4)
    pot = c["nav"].potential()
    rng = np.random.default_rng(4)
    fp = lom.rolloutFootprintRectangle(300, 200, 150, 100, True)
    states, cmd = states_of(cost, rng, 6), commands_of(rng, 50, 2)
    want = RO.evaluate_fast(cost, pot, states, cmd, fp, lom.visibilityTable(RO.TABLE), G.C_RP)
    picks, summary = c["roll"].evaluateFromGrids(c["clear"], c["nav"], states, cmd, fp, RO.as_tuple(G.C_RP))
    assert not want["error"] and summary == want["summary"] and picks.tobytes() == want["picks"].tobytes()
    assert c["roll"].records().tobytes() == want["records"].tobytes()


def test_refusals_change_nothing_and_zero_the_summary(lom):
    w, h = 65, 33
    rng = np.random.default_rng(31)
    plane, other = S.random_plane(rng, w, h), S.random_plane(rng, w, h)
    goals = first_passable(plane, P1, 3)
    dev = lom.NavField(RES, ORIGIN, w, h)
    L, sm = lom.capi.lib(), lom.capi.NavFieldSummary()
    zero = dict.fromkeys(N.SUMMARY_KEYS, 0)
    zero_shift = dict(cells_kept=0, cells_entered=0, goals_left=0)

    def refused(code, call, *args, handle=None):
        sm.cells_blocked = 9
        assert call((handle or dev).handle, *args, C.byref(sm)) == code, (call, args)
        assert sm.asdict() == zero and L.lom_navfield_last_error((handle or dev).handle)

    # before any solve
    refused(lom.capi.ERR_STATE, L.lom_navfield_shift_resolve, 1, 0, other.ctypes.data, None)
    refused(lom.capi.ERR_STATE, L.lom_navfield_shift_resolve, 0, 0, other.ctypes.data, None)
    assert (dev.potential() == N.UNREACHED).all() and dev.resolveStats() == ZERO_STATS and dev.shiftStats() == zero_shift
    assert GS.geometry_bits(dev.geometry()) == GS.geometry_bits(geo_of(w, h))
    first = dev.solve(plane, as_tuple(P1), goals)
    ref = SR.shift_resolve(geo_of(w, h), plane, other, (5, 5, 20, 20), P1, dev.potential(), 2, -1)
    check_state(dev, ref, ref["geo"], dev.shiftResolve(2, -1, other, (5, 5, 20, 20)), 0, "before the refusals")
    before, stats, paths = dev.potential(), (dev.resolveStats(), dev.shiftStats()), dev.paths(goals + 7, 30)
    assert stats[0]["cells_changed"] > 100 and first["goals_used"] == 3
    clear_other = lom.ClearanceGrid(RES, ORIGIN, w + 1, h)
    for d in ((3, 1), (0, 0)):
        refused(lom.capi.ERR_ARG, L.lom_navfield_shift_resolve, *d, None, None)
        refused(lom.capi.ERR_ARG, L.lom_navfield_shift_resolve_device, *d, None, None, None)
        refused(lom.capi.ERR_ARG, L.lom_navfield_shift_resolve_from_clearance, *d, None, None)
        refused(lom.capi.ERR_ARG, L.lom_navfield_shift_resolve_from_clearance, *d, clear_other.handle, None)
        assert b"resolution, origin, width or height differs" in L.lom_navfield_last_error(dev.handle)
    with pytest.raises(ValueError):
        dev.shiftResolve(1, 1, other[:-1])
    after = dev.paths(goals + 7, 30)
    assert dev.potential().tobytes() == before.tobytes() and (dev.resolveStats(), dev.shiftStats()) == stats
    assert after[0].tobytes() == paths[0].tobytes() and np.array_equal(after[1], paths[1])
    assert GS.geometry_bits(dev.geometry()) == GS.geometry_bits(ref["geo"])
    # the field still follows: nothing of the refused calls stuck
    ref2 = SR.shift_resolve(ref["geo"], ref["plane"], plane, None, P1, ref["P"], -2, 1)
    check_state(dev, ref2, ref2["geo"], dev.shiftResolve(-2, 1, plane), 0, "after the refusals")
    # lom_navfield_shift still clears: geometry plus clear, and a shift-resolve behind it has no field to keep
    dev.shift(4, 4)
    assert (dev.potential() == N.UNREACHED).all()
    assert GS.geometry_bits(dev.geometry()) == GS.geometry_bits(GS.shift_geometry(ref2["geo"], 4, 4)[1])
    refused(lom.capi.ERR_STATE, L.lom_navfield_shift_resolve, 1, 1, other.ctypes.data, None)
    refused(lom.capi.ERR_STATE, L.lom_navfield_shift_resolve_device, 1, 1, other.ctypes.data, None, None)
    assert (dev.potential() == N.UNREACHED).all()
    assert GS.geometry_bits(dev.geometry()) == GS.geometry_bits(GS.shift_geometry(ref2["geo"], 4, 4)[1])


# ---- mirrors -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::NavField::shiftResolve of the C++ mirror compiles with plain g++ and leaves the bytes the reference gives"""
    exe = cpp_program.build_with_library(tmp_path, "test_navfield_shift_mirror.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    lines = stdout.strip().split("\n")
    got_summary = [int(v) for v in lines[-3].split()]
    got_stats = [int(v) for v in lines[-2].split()]
    got_field = np.array([int(v) for v in lines[-1].split()], np.uint64).astype(np.uint32)
    # the same grid, planes, goals, shift and window here (tests/cpp/test_navfield_shift_mirror.cpp)
    w, h = 45, 37
    i = np.arange(w * h)
    kept = np.where(i % 7 == 3, 100, np.where(i % 5 == 0, -1, (i % 13) * 7)).astype(np.int8).reshape(h, w)
    new = np.where(i % 11 == 2, 100, (i % 9) * 5).astype(np.int8).reshape(h, w)
    goals = np.array([(0, 0), (44, 36), (20, 20)], np.int32)
    p, window = N.params(20, 2, 300, 80, N.UNKNOWN_PASSABLE), (10, 8, 30, 40)
    first = N.solve(geo_of(w, h), kept, p, goals)
    ref = SR.shift_resolve(geo_of(w, h), kept, new, window, p, first["P"], 6, -5)
    assert got_summary == [ref["summary"][k] for k in N.SUMMARY_KEYS]
    assert got_stats == [ref["cells_changed"], ref["cells_raised"], ref["cells_kept"], ref["cells_entered"], ref["goals_left"]]
    assert ref["cells_changed"] > 300 and ref["goals_left"] == 2
    assert got_field.tobytes() == ref["P"].tobytes()
