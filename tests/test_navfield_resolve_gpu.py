"""The re-solve of the navigation field on the device against tests/navfield_resolve_ref.py: after a solve of the kept plane
and a re-solve over a window of a new plane, the field as bytes, the summary, cells_changed, the paths and the query equal
the reference's full solve of the merged plane for the derived goals, under every form (raise then relax, the threshold, the
full solve from the kept goals) and every setting of the test switches; under the default form cells_raised is the size of
the least raised set.  Every case hands over garbage outside its window.  The references of a case are computed once and
shared."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_resolve_ref as RR
from tests import navfield_scenes as S

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)
P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 31), (65, 33), (129, 65)]   # the tile is 32 x 32: the last three have tile borders and a corner
FORMS = (0, 1, 2)
# inner cap (0: the default), all tiles; the batch is the default but on one shape
SWITCHES = [(cap, every) for cap in (1, 0) for every in (0, 1)]
ZERO_STATS = dict(cells_changed=0, cells_raised=0, raise_launches=0, relax_launches=0, waits=0, tiles_marked=0)
REFS = {}


def geo_of(w, h):
    return N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)


def as_tuple(p):
    return (p["neutral"], p["factor"], p["unknown_cost"], p["max_passable"], p["flags"])


def set_switches(lom, dev, form, cap, every, batch=0):
    dev.setOption(lom.capi.NAV_OPT_TEST_RESOLVE_FORM, form)
    dev.setOption(lom.capi.NAV_OPT_TEST_INNER_CAP, cap)
    dev.setOption(lom.capi.NAV_OPT_TEST_ALL_TILES, every)
    dev.setOption(lom.capi.NAV_OPT_TEST_BATCH, batch)


def given_plane(w, h, new, window, seed=99):
    """what the caller hands over: the new plane inside the window, garbage outside it (all of the new plane for None)"""
    if window is None:
        return new.copy()
    out = S.random_plane(np.random.default_rng(seed), w, h, obstacles=0.5)
    r = RR.clip(w, h, window)
    if r is not None:
        xa, ya, xb, yb = r
        out[ya:yb, xa:xb] = new[ya:yb, xa:xb]
    return out


def put(plane, x, y, value):
    """a copy with one cell set, where the cell exists"""
    out = plane.copy()
    if 0 <= x < out.shape[1] and 0 <= y < out.shape[0]:
        out[y, x] = value
    return out


def first_passable(plane, p, n):
    """n passable cells spread over the grid, the first one first, as goals (fewer where there are fewer)"""
    t = np.array(N.cell_costs(p))
    cells = np.argwhere(t[plane.view(np.uint8)] != 0)[:, ::-1].astype(np.int32).reshape(-1, 2)
    return cells[np.unique(np.linspace(0, len(cells) - 1, n).astype(int))] if len(cells) else cells


def cases_of(w, h):
    """name -> (kept plane, params, goals, new plane, window) for a shape"""
    rng = np.random.default_rng(1000 * w + h)
    origin = np.array([(0, 0)], np.int32)
    rnd, other = S.random_plane(rng, w, h, obstacles=0.1), S.random_plane(rng, w, h, obstacles=0.1)
    goals3 = first_passable(rnd, P1, 3)
    serp = S.serpentine(w, h)
    bx, by = (w // 2, 0) if w > 1 else (0, h // 2)                     # a cell of the serpentine's only route
    serp_cut = put(serp, bx, by, 100)
    passable = (rnd >= 0) & (rnd <= 90)
    dearer, cheaper = rnd.copy(), rnd.copy()
    dearer[passable] = np.minimum(rnd[passable].astype(int) + 25, 90).astype(np.int8)
    cheaper[passable] = np.maximum(rnd[passable].astype(int) - 25, 0).astype(np.int8)
    quarter = (w // 4, h // 4, max(w // 2, 1), max(h // 2, 1))
    pocket = S.pocket(w, h)
    px, py = w // 3, h // 3 + 1                                         # a cell of the pocket's wall (the pocket is cut on a tiny grid)
    rooms, door = S.two_rooms(w, h, h // 2), (w // 2, h // 2)
    # the corner rule: (1, 0) and (0, 1) are dear, (2, 0) and (0, 2) walls, so (1, 0) lies on no route and yet carries the
    # diagonal step (1, 1) -> (0, 0); blocking it takes only that step away
    diag = S.empty(w, h)
    for x, y, v in ((1, 0, 98), (0, 1, 98), (2, 0, 100), (0, 2, 100)):
        diag = put(diag, x, y, v)
    corner = rnd.copy()
    corner[31:33, 31:33] = np.array([[100, 0], [0, 100]], np.int8)[:max(0, min(h, 33) - 31), :max(0, min(w, 33) - 31)]
    g1 = goals3[:1]
    on_goal = lambda g: (int(g[0][0]), int(g[0][1]), 1, 1) if len(g) else (0, 0, 1, 1)
    blocked_goal = put(rnd, *(on_goal(g1)[:2]), 100)
    return {
        "serpentine_route_blocked": (serp, P0, origin, serp_cut, (bx, by, 1, 1)),
        "serpentine_route_freed": (serp_cut, P0, origin, serp, (bx, by, 1, 1)),
        "costs_raised": (rnd, P1, goals3, dearer, quarter),
        "costs_lowered": (rnd, P1, goals3, cheaper, quarter),
        "pocket_opened": (pocket, P0, origin, put(pocket, px, py, 0), (px - 1, py - 1, 3, 3)),
        "pocket_closed": (put(pocket, px, py, 0), P0, origin, pocket, (px - 1, py - 1, 3, 3)),
        "door_closed": (rooms, P0, origin, put(rooms, *door, 100), (*door, 1, 1)),
        "door_opened": (put(rooms, *door, 100), P0, origin, rooms, (*door, 1, 1)),
        "corner_rule": (diag, P0, origin, put(diag, 1, 0, 100), (1, 0, 1, 1)),
        "tile_corner": (rnd, P1, goals3, corner, (31, 31, 2, 2)),          # (wholly outside the smaller grids)
        "goal_blocked_one_goal": (rnd, P1, g1, blocked_goal, on_goal(g1)),
        "goal_blocked_one_of_three": (rnd, P1, goals3, blocked_goal, on_goal(g1)),
        "window_partly_outside": (rnd, P1, goals3, other, (w - 4, h - 3, 10, 10)),
        "window_partly_outside_low": (rnd, P1, goals3, other, (-5, -7, 9, 12)),
        "window_outside": (rnd, P1, goals3, other, (w, 0, 5, 5)),
        "window_empty": (rnd, P1, goals3, other, (0, 0, 0, 5)),
        "whole_grid": (rnd, P1, goals3, other, None),
        "whole_grid_to_walls": (rnd, P1, goals3, np.full((h, w), 100, np.int8), None),
        "same_plane": (rnd, P1, goals3, rnd, None),
        "same_plane_in_a_window": (rnd, P1, goals3, rnd, quarter),
    }


def references(key, w, h, kept, p, goals, new, window):
    """(the solve of the kept plane, the re-solve) of a case, once"""
    if key not in REFS:
        first = N.solve(geo_of(w, h), kept, p, goals)
        REFS[key] = (first, RR.resolve(geo_of(w, h), kept, new, window, p, first["P"]))
    return REFS[key]


def check_resolve(dev, ref, given, window, form, what, device_summary=None):
    """a re-solve of `given` over `window` on a field that holds the kept state, against the reference"""
    summary = dev.resolve(given, window) if device_summary is None else device_summary
    got, st = dev.potential(), dev.resolveStats()
    assert got.tobytes() == ref["P"].tobytes(), (what, np.argwhere(got != ref["P"])[:10])
    assert summary == ref["summary"], (what, summary, ref["summary"])
    if RR.clip(got.shape[1], got.shape[0], window) is None:
        assert st == ZERO_STATS, (what, st)
        return st
    assert st["cells_changed"] == ref["cells_changed"], (what, st)
    if ref["cells_changed"] == 0:                                       # one wait for the diff, nothing behind it
        assert st == dict(ZERO_STATS, waits=1), (what, st)
        return st
    assert st["relax_launches"] >= 1 and st["waits"] >= 3 and st["tiles_marked"] <= np.prod([-(-v // 32) for v in got.shape])
    if form == 0:
        assert st["cells_raised"] == ref["cells_raised"] and st["raise_launches"] >= 1, (what, st, ref["cells_raised"])
    else:
        assert st["raise_launches"] == 0 and st["cells_raised"] >= (ref["cells_raised"] if form == 1 else 0), (what, st)
    return st


def check_reads(dev, ref, w, h, rng, what):
    """paths and the query read the new state"""
    geo = geo_of(w, h)
    starts = np.concatenate([np.stack([rng.integers(0, w, 6), rng.integers(0, h, 6)], axis=1),
                             np.array([(0, 0), (w - 1, h - 1), (-1, 0), (w, h - 1)])]).astype(np.int32)
    cells, lengths = dev.paths(starts, 40)
    want_cells, want_lengths = N.paths(geo, ref["costs"], ref["P"], starts, 40)
    assert np.array_equal(lengths, want_lengths) and cells.tobytes() == want_cells.tobytes(), what
    xy = np.concatenate([rng.uniform(ORIGIN[0] - 1.0, ORIGIN[0] + w * RES + 1.0, (40, 1)),
                         rng.uniform(ORIGIN[1] - 1.0, ORIGIN[1] + h * RES + 1.0, (40, 1))], axis=1).astype(np.float32)
    assert np.array_equal(dev.query(xy), N.query(geo, ref["P"], xy)), what


# ---- 1: shapes x cases x forms x switches --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_cases_forms_and_switches(lom, w, h):
    rng = np.random.default_rng(w + 7 * h)
    dev = lom.NavField(RES, ORIGIN, w, h)
    batches = (1, 8, 0) if (w, h) == (65, 33) else (0,)
    for name, (kept, p, goals, new, window) in cases_of(w, h).items():
        first, ref = references((w, h, name), w, h, kept, p, goals, new, window)
        given = given_plane(w, h, new, window)
        assert np.array_equal(RR.merged_plane(kept, given, window), ref["plane"]) and not first["error"]
        raised = {}
        for form in FORMS:
            for cap, every in SWITCHES:
                for batch in batches:
                    set_switches(lom, dev, form, 0, 0)                   # (the solve in front is not what the case is about)
                    assert dev.solve(kept, as_tuple(p), goals) == first["summary"]
                    set_switches(lom, dev, form, cap, every, batch)
                    st = check_resolve(dev, ref, given, window, form, (name, form, cap, every, batch))
                    raised.setdefault(form, st["cells_raised"])
                    assert st["cells_raised"] == raised[form], (name, form, cap, every, batch)   # of the form, not of the schedule
        check_reads(dev, ref, w, h, rng, name)
        # a second re-solve of the same plane finds nothing changed: the kept plane is the merged one
        again = dev.resolve(ref["plane"], None)
        assert again == dict(ref["summary"], goals_used=ref["summary"]["goals_used"], goals_rejected=0), name
        assert dev.resolveStats() == dict(ZERO_STATS, waits=1) and dev.potential().tobytes() == ref["P"].tobytes()
    # what the cases are for, on the reference
    if (w, h) == (129, 65):
        r = {name: REFS[(w, h, name)] for name in cases_of(w, h)}
        n_route = int((S.serpentine(w, h) == 0).sum())
        assert r["serpentine_route_blocked"][1]["summary"]["cells_reached"] == w // 2
        assert r["serpentine_route_blocked"][1]["cells_raised"] == n_route - w // 2 - 1
        assert r["serpentine_route_freed"][1]["cells_raised"] == 0 and r["serpentine_route_freed"][1]["summary"]["cells_unreached"] == 0
        assert r["costs_raised"][1]["cells_raised"] > 100 and r["costs_lowered"][1]["cells_raised"] == 0
        assert r["costs_lowered"][1]["P"].tobytes() != r["costs_lowered"][0]["P"].tobytes()
        assert r["pocket_opened"][0]["summary"]["cells_unreached"] > 0 and r["pocket_opened"][1]["summary"]["cells_unreached"] == 0
        assert r["pocket_closed"][1]["cells_raised"] == r["pocket_opened"][0]["summary"]["cells_unreached"]
        assert r["door_closed"][1]["cells_raised"] == (w - w // 2 - 1) * h and r["door_opened"][1]["cells_raised"] == 0
        assert r["corner_rule"][1]["cells_changed"] == 1 and r["corner_rule"][1]["cells_raised"] > 1000
        assert r["corner_rule"][0]["P"][1, 1] == 7 * 50 and r["corner_rule"][1]["P"][1, 1] == 5 * 50 + 5 * (50 + 3 * 98)
        assert r["tile_corner"][1]["cells_changed"] >= 2
        s = r["goal_blocked_one_goal"][1]["summary"]
        assert (s["goals_used"], s["goals_rejected"], s["cells_reached"]) == (0, 1, 0)
        s = r["goal_blocked_one_of_three"][1]["summary"]
        assert (s["goals_used"], s["goals_rejected"]) == (2, 1) and s["cells_reached"] > 1000
        assert 0 < r["window_partly_outside"][1]["cells_changed"] <= 12 and r["window_outside"][1]["cells_changed"] == 0
        assert r["whole_grid"][1]["cells_changed"] > 7000 and r["whole_grid_to_walls"][1]["summary"]["goals_rejected"] == 3


def test_the_default_form_does_less_than_the_full_solve_far_from_the_goal(lom):
    """a wall cell next to the far corner of free ground: the least set is a handful of cells, and the relaxation that
    follows touches one tile's neighbourhood, not the grid"""
    w, h = 129, 65
    kept = S.empty(w, h)
    new = put(kept, w - 3, h - 3, 100)
    goals, window = np.array([(0, 0)], np.int32), (w - 3, h - 3, 1, 1)
    first, ref = references("far", w, h, kept, P0, goals, new, window)
    dev = lom.NavField(RES, ORIGIN, w, h)
    stats = {}
    for form in FORMS:
        set_switches(lom, dev, form, 0, 0, batch=1)                     # a wait per launch: the counts are exact
        dev.solve(kept, as_tuple(P0), goals)
        stats[form] = check_resolve(dev, ref, given_plane(w, h, new, window), window, form, form)
    assert ref["cells_raised"] <= 8 and stats[0]["cells_raised"] == ref["cells_raised"] <= stats[1]["cells_raised"]
    assert stats[0]["tiles_marked"] <= 4 and stats[0]["relax_launches"] < stats[2]["relax_launches"]


# ---- 2: the range --------------------------------------------------------------------------------------------------------------
def test_range_exceeded_on_the_serpentine(lom):
    """neutral = 2^24 - 1 on the serpentine: the values pass LOM_NAV_MAX 51 steps from the goal.  A wall inside the reach cuts
    it short; taking it out again restores the flag and the 52 cells"""
    w, h = 129, 65
    plane = S.serpentine(w, h)
    p = N.params(N.MAX_CELL_COST, 0, 1, 98)
    goals, window = np.array([(0, 0)], np.int32), (30, 0, 1, 1)
    cut = put(plane, 30, 0, 100)
    first, ref = references("range_cut", w, h, plane, p, goals, cut, window)
    assert first["summary"]["range_exceeded"] == 1 and first["summary"]["cells_reached"] == 52
    assert ref["summary"]["range_exceeded"] == 0 and ref["summary"]["cells_reached"] == 30 and ref["cells_raised"] == 21
    first_back, back = references("range_back", w, h, cut, p, goals, plane, window)
    assert back["summary"] == dict(first["summary"]) and back["P"].tobytes() == first["P"].tobytes() and back["cells_raised"] == 0
    dev = lom.NavField(RES, ORIGIN, w, h)
    for form in FORMS:
        for cap, every in SWITCHES:
            set_switches(lom, dev, form, cap, every)
            assert dev.solve(plane, as_tuple(p), goals) == first["summary"]
            check_resolve(dev, ref, given_plane(w, h, cut, window), window, form, ("cut", form, cap, every))
            check_resolve(dev, back, given_plane(w, h, plane, window), window, form, ("back", form, cap, every))


# ---- 3: a chain of re-solves on one handle ---------------------------------------------------------------------------------------
def test_a_chain_of_twelve_resolves(lom):
    """random windows of random planes, one after another on one handle per form: each equals the reference's re-solve of the
    plane as merged so far -- a stale kept plane, stale marks or a wrong launch parity would show"""
    w, h = 65, 33
    rng = np.random.default_rng(77)
    geo = geo_of(w, h)
    kept = S.random_plane(rng, w, h, obstacles=0.2)
    goals = first_passable(kept, P1, 3)
    first = N.solve(geo, kept, P1, goals)
    devs = {form: lom.NavField(RES, ORIGIN, w, h) for form in FORMS}
    for form, dev in devs.items():
        set_switches(lom, dev, form, 0, 0)
        assert dev.solve(kept, as_tuple(P1), goals) == first["summary"]
    P_old, changed = first["P"], 0
    for k in range(12):
        window = (int(rng.integers(-4, w)), int(rng.integers(-4, h)), int(rng.integers(1, 24)), int(rng.integers(1, 24)))
        new = S.random_plane(rng, w, h, obstacles=float(rng.choice([0.0, 0.2, 0.6])))
        ref = RR.resolve(geo, kept, new, window, P1, P_old)
        for form, dev in devs.items():
            if k % 4 == 3:
                set_switches(lom, dev, form, 1, k % 8 == 7)
            check_resolve(dev, ref, given_plane(w, h, new, window, seed=k), window, form, (k, form))
        kept, P_old, changed = ref["plane"], ref["P"], changed + ref["cells_changed"]
    assert changed > 300 and ref["summary"]["cells_reached"] > 100
    check_reads(devs[0], ref, w, h, rng, "chain")


# ---- 4: refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_zero_the_summary(lom):
    w, h = 65, 33
    rng = np.random.default_rng(31)
    plane, other = S.random_plane(rng, w, h), S.random_plane(rng, w, h)
    goals = first_passable(plane, P1, 3)
    dev = lom.NavField(RES, ORIGIN, w, h)
    L, sm = lom.capi.lib(), lom.capi.NavFieldSummary()
    zero = dict.fromkeys(N.SUMMARY_KEYS, 0)

    def refused(code, call, *args):
        sm.cells_blocked = 9
        assert call(dev.handle, *args, C.byref(sm)) == code
        assert sm.asdict() == zero and L.lom_navfield_last_error(dev.handle)

    # before any solve, and after a clear
    refused(lom.capi.ERR_STATE, L.lom_navfield_resolve, other.ctypes.data, None)
    with pytest.raises(lom.LomError) as e:
        dev.resolve(other)
    assert e.value.code == lom.capi.ERR_STATE and (dev.potential() == N.UNREACHED).all() and dev.resolveStats() == ZERO_STATS
    first = dev.solve(plane, as_tuple(P1), goals)
    ref = RR.resolve(geo_of(w, h), plane, other, (5, 5, 20, 20), P1, dev.potential())
    check_resolve(dev, ref, other, (5, 5, 20, 20), 0, "before the refusals")
    before, stats, paths = dev.potential(), dev.resolveStats(), dev.paths(goals + 7, 30)
    assert stats["cells_changed"] > 100 and first["goals_used"] == 3
    clear_other = lom.ClearanceGrid(RES, ORIGIN, w + 1, h)
    refused(lom.capi.ERR_ARG, L.lom_navfield_resolve, None, None)
    refused(lom.capi.ERR_ARG, L.lom_navfield_resolve_device, None, None, None)
    refused(lom.capi.ERR_ARG, L.lom_navfield_resolve_from_clearance, None, None)
    refused(lom.capi.ERR_ARG, L.lom_navfield_resolve_from_clearance, clear_other.handle, None)
    assert b"resolution, origin, width or height differs" in L.lom_navfield_last_error(dev.handle)
    with pytest.raises(ValueError):
        dev.resolve(other[:-1])
    with pytest.raises(lom.LomError):
        dev.setOption(lom.capi.NAV_OPT_TEST_RESOLVE_FORM, 3)
    after = dev.paths(goals + 7, 30)
    assert dev.potential().tobytes() == before.tobytes() and dev.resolveStats() == stats
    assert after[0].tobytes() == paths[0].tobytes() and np.array_equal(after[1], paths[1])
    # the field still re-solves: nothing of the refused calls stuck
    ref2 = RR.resolve(geo_of(w, h), ref["plane"], plane, None, P1, ref["P"])
    check_resolve(dev, ref2, plane, None, 0, "after the refusals")
    dev.clear()
    refused(lom.capi.ERR_STATE, L.lom_navfield_resolve, other.ctypes.data, None)
    refused(lom.capi.ERR_STATE, L.lom_navfield_resolve_device, other.ctypes.data, None, None)
    assert (dev.potential() == N.UNREACHED).all()


# ---- 5: from the clearance grid, and the device form -------------------------------------------------------------------------------
def test_resolve_from_clearance_behind_a_windowed_update(lom):
    """a stream per handle: the clearance grid updates a window, the field re-solves the same window, three times over; each
    equals the references' chain (tests/clearance_ref.py, then the re-solve of its cost plane)"""
    rng = np.random.default_rng(23)
    w, h = 65, 33
    cgeo, geo = K.geometry(RES, ORIGIN[0], ORIGIN[1], w, h), geo_of(w, h)
    clear, dev = lom.ClearanceGrid(RES, ORIGIN, w, h), lom.NavField(RES, ORIGIN, w, h)
    occ = np.where(rng.random((h, w)) < 0.03, 100, 0).astype(np.int8)
    cp = K.params(1.0, 0.3, 1.5)
    table, state = lom.clearanceCostTable(cp, RES), K.empty_state(cgeo)
    clear.update(occ, None, cp)
    want = K.update(cgeo, occ, None, cp, None, state, table)
    state = dict(d2=want["d2"], cost=want["cost"])
    goals = first_passable(want["cost"], P0, 2)
    assert dev.solveFromClearance(clear, as_tuple(P0), goals) == N.solve(geo, want["cost"], P0, goals)["summary"]
    kept, P_old = want["cost"], dev.potential()
    for k, window in enumerate(((40, 10, 20, 16), (-3, 20, 30, 30), (30, 0, 9, 9))):
        r = RR.clip(w, h, window)
        occ = occ.copy()
        occ[r[1]:r[3], r[0]:r[2]] = np.where(rng.random((r[3] - r[1], r[2] - r[0])) < (0.15, 0.0, 0.3)[k], 100, 0)
        clear.update(occ, None, cp, window=window)
        want = K.update(cgeo, occ, None, cp, window, state, table)
        state = dict(d2=want["d2"], cost=want["cost"])
        ref = RR.resolve(geo, kept, want["cost"], window, P0, P_old)
        check_resolve(dev, ref, None, window, 0, k, device_summary=dev.resolveFromClearance(clear, window))
        assert np.array_equal(clear.cost()[0], ref["plane"]) and ref["cells_changed"] > 0, k
        kept, P_old = ref["plane"], ref["P"]


def test_device_form_and_a_callers_event(lom):
    import torch

    rng = np.random.default_rng(12)
    w, h = 129, 65
    kept, new = S.random_plane(rng, w, h, obstacles=0.2), S.random_plane(rng, w, h, obstacles=0.3)
    goals, window = first_passable(kept, P1, 3), (20, 10, 60, 40)
    first, ref = references("device_form", w, h, kept, P1, goals, new, window)
    dev = lom.NavField(RES, ORIGIN, w, h)
    d_field = C.c_void_p()
    assert dev.solve(kept, as_tuple(P1), goals) == first["summary"]
    assert lom.capi.lib().lom_navfield_potential_device(dev.handle, C.byref(d_field)) == 0
    # a plane produced on another stream: the re-solve waits for the caller's event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.ones(1 << 24, device="cuda:0")
        for _ in range(10):                                          # work in front of the plane
            big = big * 1.0001 + 1.0
        u = torch.from_numpy(given_plane(w, h, new, window)).to("cuda:0", non_blocking=True) + 0
        ev = torch.cuda.Event()
        ev.record(s)
    summary = dev.resolve(u.data_ptr(), window, device=True, hip_event=C.c_void_p(ev.cuda_event))
    check_resolve(dev, ref, None, window, 0, "device form", device_summary=summary)
    # the pointer of the potential stays valid across the call, and the field keeps its own copy of the plane
    again = C.c_void_p()
    assert lom.capi.lib().lom_navfield_potential_device(dev.handle, C.byref(again)) == 0 and again.value == d_field.value
    u.fill_(100)
    torch.cuda.synchronize()
    check_reads(dev, ref, w, h, rng, "device form")
    # no event: the plane is complete now
    t = torch.from_numpy(given_plane(w, h, kept, None)).to("cuda:0")
    torch.cuda.synchronize()
    back = RR.resolve(geo_of(w, h), ref["plane"], kept, None, P1, ref["P"])
    check_resolve(dev, back, None, None, 0, "device form, whole grid", device_summary=dev.resolve(t.data_ptr(), None, device=True))
    torch.cuda.synchronize()


# ---- 6: the planning chain with a re-solve in its second round -------------------------------------------------------------------
def test_the_chain_with_a_resolve_in_its_second_round(lom):
    """tests/test_plane_core_gpu.py's chain on five streams; in the second round the field is re-solved from the clearance grid
    instead of solved, and every consumer behind the field equals its reference over the re-solved potential"""
    from tests import regions_ref as R
    from tests import visibility_ref as V
    from tests import test_plane_core_gpu as T

    c = T.Chain(lom)
    first = c.round(0)
    c.occ.integrateCloud(c.scans[1], T.POSES[1], T.RAY)
    c.elev.integrateCloud(c.scans[1], T.POSES[1], T.PNT)
    got = dict(clear=c.clear.updateFromGrids(c.occ, T.RULE, c.elev, T.LAYER, T.COSTP, T.CP),
               nav=c.nav.resolveFromClearance(c.clear),
               reg=c.reg.extractFromGrids(c.occ, T.RULE, c.clear, c.nav, R.as_tuple(T.RP)),
               vis=c.vis.castFromOccupancy(c.occ, T.RULE, T.VP, V.as_tuple(T.VISP)),
               picks=c.vis.selectFromNavfield(c.nav, V.select_tuple(T.SEL)))
    back = c.read()
    occ, elev, cost, pot = back["occ"], back["elev"], back["cost"], back["potential"]
    ref = K.update(T.GEO, occ, elev, T.CP, None, c.state, c.table)
    assert got["clear"] == ref["summary"] and np.array_equal(cost, ref["cost"])
    ref = RR.resolve(T.GEO, first["cost"], cost, None, N.params(*T.NP), first["potential"])
    assert got["nav"] == ref["summary"] and pot.tobytes() == ref["P"].tobytes(), (got["nav"], ref["summary"])
    assert ref["cells_changed"] > 0 and pot.tobytes() != first["potential"].tobytes()
    assert c.nav.resolveStats()["cells_changed"] == ref["cells_changed"] and c.nav.resolveStats()["cells_raised"] == ref["cells_raised"]
    ref = R.extract(occ, T.RP, cost, pot)
    assert got["reg"] == ref["summary"] and back["labels"].tobytes() == ref["labels"].tobytes() and back["list"].tobytes() == ref["list"].tobytes()
    ref = V.cast_fast(occ, T.VP, c.beams, T.VISP)
    assert got["vis"] == ref["summary"] and back["records"].tobytes() == ref["records"].tobytes()
    assert got["picks"].tobytes() == V.select(ref, T.SEL, pot[T.VP[:, 1], T.VP[:, 0]]).tobytes()
    # the rollouts read the re-solved potential in place
    from tests import rollout_ref as RO
    from tests.rollout_scenes import commands_of, states_of
    rng = np.random.default_rng(4)
    fp = lom.rolloutFootprintRectangle(300, 200, 150, 100, True)
    states, cmd = states_of(cost, rng, 6), commands_of(rng, 50, 2)
    p = RO.params(2, 40, 99, 30, min_steps=10, progress_weight=4, cost_weight=1, truncation_weight=100)
    want = RO.evaluate_fast(cost, pot, states, cmd, fp, lom.visibilityTable(RO.TABLE), p)
    roll = lom.RolloutGrid(T.RES, T.ORG, T.W, T.H)
    picks, summary = roll.evaluateFromGrids(c.clear, c.nav, states, cmd, fp, RO.as_tuple(p))
    assert not want["error"] and summary == want["summary"] and picks.tobytes() == want["picks"].tobytes()
    assert roll.records().tobytes() == want["records"].tobytes()


# ---- mirrors -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::NavField::resolve of the C++ mirror compiles with plain g++ and leaves the bytes the Python package leaves."""
    exe = cpp_program.build_with_library(tmp_path, "test_navfield_resolve_mirror.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    lines = stdout.strip().split("\n")
    got_summary = [int(v) for v in lines[-3].split()]
    got_stats = [int(v) for v in lines[-2].split()]
    got_field = np.array([int(v) for v in lines[-1].split()], np.uint64).astype(np.uint32)
    # the same grid, planes, goals and window here (tests/cpp/test_navfield_resolve_mirror.cpp)
    w, h = 45, 37
    i = np.arange(w * h)
    kept = np.where(i % 7 == 3, 100, np.where(i % 5 == 0, -1, (i % 13) * 7)).astype(np.int8).reshape(h, w)
    new = np.where(i % 11 == 2, 100, (i % 9) * 5).astype(np.int8).reshape(h, w)
    goals = np.array([(0, 0), (44, 36), (20, 20)], np.int32)
    p, window = N.params(20, 2, 300, 80, N.UNKNOWN_PASSABLE), (10, 8, 30, 40)
    first = N.solve(geo_of(w, h), kept, p, goals)
    ref = RR.resolve(geo_of(w, h), kept, new, window, p, first["P"])
    assert got_summary == [ref["summary"][k] for k in N.SUMMARY_KEYS]
    assert got_stats == [ref["cells_changed"], ref["cells_raised"]] and ref["cells_changed"] > 500
    assert got_field.tobytes() == ref["P"].tobytes()
    dev = lom.NavField(RES, ORIGIN, w, h)
    dev.solve(kept, as_tuple(p), goals)
    assert dev.resolve(new, window) == ref["summary"] and dev.potential().tobytes() == got_field.tobytes()
