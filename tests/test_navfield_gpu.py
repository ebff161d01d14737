"""The navigation field on the device against tests/navfield_ref.py: the field as bytes, the summary, the paths with their
lengths and the query -- all exactly equal, under every setting of the three test switches.  The reference of a case is
computed once and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_scenes as S

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)
P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)
SHAPES = [(1, 1), (1, 70), (70, 1), (32, 32), (33, 31), (65, 33), (129, 65)]
# inner cap (0: the default), batch, all tiles
SWITCHES = [(cap, batch, every) for cap in (1, 0) for batch in (1, 8) for every in (0, 1)]
REFS = {}


def geo_of(w, h):
    return N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)


def as_tuple(p):
    return (p["neutral"], p["factor"], p["unknown_cost"], p["max_passable"], p["flags"])


def reference(key, w, h, plane, p, goals, metres=False):
    """the reference's solve of a case, once"""
    if key not in REFS:
        REFS[key] = N.solve(geo_of(w, h), plane, p, goals, metres)
    return REFS[key]


def set_switches(lom, dev, cap, batch, every):
    dev.setOption(lom.capi.NAV_OPT_TEST_INNER_CAP, cap)
    dev.setOption(lom.capi.NAV_OPT_TEST_BATCH, batch)
    dev.setOption(lom.capi.NAV_OPT_TEST_ALL_TILES, every)


def check_solve(dev, ref, plane, p, goals, metres=False, what=None):
    summary = dev.solve(plane, as_tuple(p), goals, metres=metres)
    got = dev.potential()
    assert got.tobytes() == ref["P"].tobytes(), (what, np.argwhere(got != ref["P"])[:10])
    assert summary == ref["summary"], (what, summary, ref["summary"])
    st = dev.stats()
    assert st["launches"] >= 1 and 1 <= st["waits"] <= st["launches"]


def border_goals(w, h):
    """the four corners, cells on both sides of every tile border, duplicates, and goals outside the grid"""
    g = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (0, 0), (w - 1, h - 1)]
    for v in (31, 32, 63, 64):
        g += [(v, h // 2), (w // 2, v), (v, v)]
    g += [(-1, 0), (0, -1), (w, 0), (0, h), (w + 5, h + 5), (-(2 ** 31), 2 ** 31 - 1)]
    return np.array(g, np.int64).astype(np.int32)


def some_starts(rng, w, h, n):
    """cells all over the grid, the corners, and a few outside it"""
    s = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1)
    extra = [(0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1), (-1, 0), (w, h - 1), (0, h), (3, -7)]
    return np.concatenate([s, np.array(extra)]).astype(np.int32)


def cases_of(w, h):
    """name -> (plane, params, goals) for a shape"""
    rng = np.random.default_rng(1000 * w + h)
    rnd = S.random_plane(rng, w, h)
    far = np.array([(0, 0)], np.int32)
    out = {
        "empty": (S.empty(w, h), P0, border_goals(w, h)),
        "empty_no_goal": (S.empty(w, h), P0, np.zeros((0, 2), np.int32)),
        "random": (rnd, P0, border_goals(w, h)),
        "random_unknown_passable": (rnd, P1, border_goals(w, h)),
        "random_one_goal": (rnd, P1, np.argwhere((rnd >= 0) & (rnd <= 90))[:1, ::-1].astype(np.int32)),   # (none on a tiny grid: G = 0)
        "serpentine": (S.serpentine(w, h), P0, far),
        "spiral": (S.spiral(w, h), P0, far),
        "diagonal_gaps": (S.diagonal_gaps(w, h), P0, far),
        "diagonal_gaps_many_goals": (S.diagonal_gaps(w, h), P0, border_goals(w, h)),
        "pocket": (S.pocket(w, h), P0, np.array([(0, 0), (w - 1, h - 1)], np.int32)),
        "all_blocked": (np.full((h, w), 100, np.int8), P0, border_goals(w, h)),
    }
    return out


# ---- 1: shapes x scenes x switches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_scenes_and_switches(lom, w, h):
    rng = np.random.default_rng(w + 7 * h)
    dev = lom.NavField(RES, ORIGIN, w, h)
    geo = geo_of(w, h)
    for name, (plane, p, goals) in cases_of(w, h).items():
        ref = reference((w, h, name), w, h, plane, p, goals)
        assert not ref["error"]
        for cap, batch, every in SWITCHES:
            set_switches(lom, dev, cap, batch, every)
            check_solve(dev, ref, plane, p, goals, what=(name, cap, batch, every))
        # paths and the query on what the last solve left
        starts = some_starts(rng, w, h, 6)
        cap_cells = 40
        cells, lengths = dev.paths(starts, cap_cells)
        want_cells, want_lengths = N.paths(geo, ref["costs"], ref["P"], starts, cap_cells)
        assert np.array_equal(lengths, want_lengths), (name, lengths, want_lengths)
        assert cells.tobytes() == want_cells.tobytes(), name
        xy = np.concatenate([rng.uniform(ORIGIN[0] - 1.0, ORIGIN[0] + w * RES + 1.0, (50, 1)),
                             rng.uniform(ORIGIN[1] - 1.0, ORIGIN[1] + h * RES + 1.0, (50, 1))], axis=1).astype(np.float32)
        assert np.array_equal(dev.query(xy), N.query(geo, ref["P"], xy)), name
    # what the scenes are for, on the reference
    if (w, h) == (129, 65):
        assert REFS[(w, h, "serpentine")]["summary"]["cells_unreached"] == 0
        assert REFS[(w, h, "serpentine")]["summary"]["max_potential"] == 250 * (int((S.serpentine(w, h) == 0).sum()) - 1)
        assert REFS[(w, h, "spiral")]["summary"]["max_potential"] > 250 * 2000
        assert REFS[(w, h, "pocket")]["summary"]["cells_unreached"] > 0
        assert REFS[(w, h, "random")]["summary"]["goals_rejected"] > 6 and REFS[(w, h, "random")]["summary"]["goals_used"] >= 2
        assert REFS[(w, h, "empty_no_goal")]["summary"]["cells_reached"] == 0
        # the default switches take fewer launches than one sweep per launch
        plane, p, goals = cases_of(w, h)["serpentine"]
        set_switches(lom, dev, 1, 8, 1)
        dev.solve(plane, as_tuple(p), goals)
        slow = dev.stats()["launches"]
        set_switches(lom, dev, 0, 0, 0)
        dev.solve(plane, as_tuple(p), goals)
        assert dev.stats()["launches"] < slow


def test_goals_in_metres_and_the_query_at_cell_borders(lom):
    w, h = 65, 33
    rng = np.random.default_rng(3)
    plane = S.random_plane(rng, w, h, obstacles=0.1)
    geo = geo_of(w, h)
    nan, inf = np.nan, np.inf
    goals = np.array([[-3.0, 2.0], [-2.75, 2.25], [-2.7500002, 2.2499998], [13.249999, 10.249999], [13.25, 5.0], [5.0, 10.25],
                      [-3.0000002, 5.0], [nan, 5.0], [5.0, nan], [inf, 5.0], [5.0, -inf], [4.9, 6.1], [4.9, 6.1], [1e30, -1e30]], np.float32)
    ref = reference("metres", w, h, plane, P1, goals, metres=True)
    assert ref["summary"]["goals_rejected"] >= 8 and ref["summary"]["goals_used"] >= 1
    dev = lom.NavField(RES, ORIGIN, w, h)
    check_solve(dev, ref, plane, P1, goals, metres=True)
    xy = np.concatenate([goals, rng.uniform(-5, 15, (300, 2)).astype(np.float32)])
    got, want = dev.query(xy), N.query(geo, ref["P"], xy)
    assert np.array_equal(got, want) and (want[6:11] == N.UNREACHED).all() and (want != N.UNREACHED).sum() > 50
    assert len(dev.query(np.zeros((0, 2), np.float32))) == 0
    # starts in metres
    cells, lengths = dev.paths(xy[:40], 25, metres=True)
    want_cells, want_lengths = N.paths(geo, ref["costs"], ref["P"], xy[:40], 25, metres=True)
    assert np.array_equal(lengths, want_lengths) and cells.tobytes() == want_cells.tobytes()
    L = lom.capi.lib()
    assert L.lom_navfield_query(dev.handle, None, 3, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_paths(dev.handle, 5, xy.ctypes.data, 3, cells.ctypes.data, 25, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_paths(dev.handle, 0, None, 3, cells.ctypes.data, 25, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_paths(dev.handle, 0, xy.ctypes.data, 3, None, 25, None) == lom.capi.ERR_ARG
    assert L.lom_navfield_paths(dev.handle, 0, xy.ctypes.data, 1 << 20, cells.ctypes.data, 1 << 20, None) == lom.capi.ERR_ARG


# ---- 2: the range --------------------------------------------------------------------------------------------------------------
def test_range_exceeded_on_the_serpentine(lom):
    """neutral = 2^24 - 1: an axial step weighs 5 * (2^24 - 1), so the values pass LOM_NAV_MAX 51 steps from the goal; the
    cells beyond read unreached, those before are exact"""
    w, h = 129, 65
    plane = S.serpentine(w, h)
    p = N.params(N.MAX_CELL_COST, 0, 1, 98)
    goals = np.array([(0, 0)], np.int32)
    ref = reference("range", w, h, plane, p, goals)
    s = ref["summary"]
    assert s["range_exceeded"] == 1 and s["cells_reached"] == 52 and s["cells_unreached"] == int((plane == 0).sum()) - 52
    assert ref["P"][0, 51] == 51 * 5 * N.MAX_CELL_COST and ref["P"][0, 52] == N.UNREACHED
    dev = lom.NavField(RES, ORIGIN, w, h)
    for cap, batch, every in SWITCHES:
        set_switches(lom, dev, cap, batch, every)
        check_solve(dev, ref, plane, p, goals, what=(cap, batch, every))
    # one cell short of the range: every step fits, the flag stays down
    short = plane.copy()
    short[0, 51:] = 100
    short[1:, :] = 100
    ref = reference("range_short", w, h, short, p, goals)
    assert ref["summary"]["range_exceeded"] == 0 and ref["summary"]["cells_reached"] == 51
    check_solve(dev, ref, short, p, goals)


# ---- 3: paths ------------------------------------------------------------------------------------------------------------------
def test_paths_caps_and_starts(lom):
    w, h = 65, 33
    geo = geo_of(w, h)
    plane = S.pocket(w, h)
    plane[5, 10:40] = 60
    goals = np.array([(2, 3)], np.int32)
    ref = reference("paths", w, h, plane, P0, goals)
    dev = lom.NavField(RES, ORIGIN, w, h)
    check_solve(dev, ref, plane, P0, goals)
    inside = (w // 3 + 1, h // 3 + 1)
    assert ref["P"][inside[1], inside[0]] == N.UNREACHED and plane[inside[1], inside[0]] == 0
    far = (w - 1, h - 1)
    full = N.path(geo, ref["costs"], ref["P"], far)
    n = len(full)
    assert n > 30 and full[-1] == (2, 3)
    starts = np.array([far, (2, 3), inside, (-1, 5), (w, 5), (5, h), (w // 3, h // 3)], np.int32)   # ..., on a wall of the pocket
    for cap in (n - 7, n, n + 9, 1, 0):                      # smaller than, equal to, larger than the length; one cell; none
        cells, lengths = dev.paths(starts, cap)
        want_cells, want_lengths = N.paths(geo, ref["costs"], ref["P"], starts, cap)
        assert lengths.tolist() == want_lengths.tolist() == [n, 1, 0, 0, 0, 0, 0], cap
        assert cells.shape == (7, cap, 2) and cells.tobytes() == want_cells.tobytes(), cap
        if cap >= n:
            assert [tuple(int(v) for v in c) for c in cells[0, :n]] == full and (cells[0, n:] == 0).all()
    # K = 1 and K = 200
    rng = np.random.default_rng(8)
    for k in (1, 200):
        s = some_starts(rng, w, h, k)[:k]
        cells, lengths = dev.paths(s, 16)
        want_cells, want_lengths = N.paths(geo, ref["costs"], ref["P"], s, 16)
        assert np.array_equal(lengths, want_lengths) and cells.tobytes() == want_cells.tobytes()
    cells, lengths = dev.paths(np.zeros((0, 2), np.int32), 16)
    assert cells.shape == (0, 16, 2) and len(lengths) == 0
    # every device path sums to P[start] over allowed steps
    cells, lengths = dev.paths(starts[:1], n)
    route = [tuple(int(v) for v in c) for c in cells[0, :lengths[0]]]
    assert N.path_weight(ref["costs"], route) == int(ref["P"][far[1], far[0]])


# ---- 4: from the clearance grid --------------------------------------------------------------------------------------------------
def test_solve_from_clearance(lom):
    rng = np.random.default_rng(21)
    w, h = 130, 67
    clear = lom.ClearanceGrid(RES, ORIGIN, w, h)
    occ = np.where(rng.random((h, w)) < 0.03, 100, rng.choice(np.array([0, -1], np.int8), (h, w))).astype(np.int8)
    elev = rng.integers(-1, 70, (h, w)).astype(np.int8)
    cp = K.params(1.0, 0.3, 1.5)
    goals = border_goals(w, h)
    dev = lom.NavField(RES, ORIGIN, w, h)
    host = lom.NavField(RES, ORIGIN, w, h)
    for p in (P0, P1):
        clear.update(occ, elev, cp)
        cost = clear.cost()[0]
        assert (cost == 100).any() and (cost == 99).any() and ((cost > 0) & (cost < 99)).any()
        got = dev.solveFromClearance(clear, as_tuple(p), goals)
        want = host.solve(cost, as_tuple(p), goals)
        assert got == want and dev.potential().tobytes() == host.potential().tobytes()
        ref = reference(("clearance", p["flags"]), w, h, cost, p, goals)
        assert got == ref["summary"] and dev.potential().tobytes() == ref["P"].tobytes()
        occ = np.roll(occ, 7, axis=1)                                   # the clearance grid goes on: another plane next time
    # a clearance grid of another geometry is refused, and nothing changes
    before = dev.potential()
    others = [lom.ClearanceGrid(RES, ORIGIN, w + 1, h), lom.ClearanceGrid(RES, ORIGIN, w, h - 1),
              lom.ClearanceGrid(RES, (ORIGIN[0] + 1e-6, ORIGIN[1]), w, h), lom.ClearanceGrid(RES, (ORIGIN[0], ORIGIN[1] - 1e-6), w, h),
              lom.ClearanceGrid(np.nextafter(np.float32(RES), np.float32(1)), ORIGIN, w, h)]
    for other in others:
        with pytest.raises(lom.LomError) as e:
            dev.solveFromClearance(other, as_tuple(P0), goals)
        assert e.value.code == lom.capi.ERR_ARG
    with pytest.raises(lom.LomError):
        dev.solveFromClearance(clear, (0, 3, 400, 98, 0), goals)
    assert dev.potential().tobytes() == before.tobytes()


def test_device_form_and_a_callers_event(lom):
    import torch

    rng = np.random.default_rng(12)
    w, h = 129, 65
    plane = S.random_plane(rng, w, h, obstacles=0.2)
    goals = border_goals(w, h)
    ref = reference("device_form", w, h, plane, P1, goals)
    dev = lom.NavField(RES, ORIGIN, w, h)
    t = torch.from_numpy(plane).to("cuda:0")
    torch.cuda.synchronize()
    assert dev.solve(t.data_ptr(), as_tuple(P1), goals, device=True) == ref["summary"]
    assert dev.potential().tobytes() == ref["P"].tobytes()
    # a plane produced on another stream: the solve waits for the caller's event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.ones(1 << 24, device="cuda:0")
        for _ in range(10):                                          # work in front of the plane
            big = big * 1.0001 + 1.0
        u = torch.from_numpy(plane).to("cuda:0", non_blocking=True) + 0
        ev = torch.cuda.Event()
        ev.record(s)
    late = lom.NavField(RES, ORIGIN, w, h)
    assert late.solve(u.data_ptr(), as_tuple(P1), goals, device=True, hip_event=C.c_void_p(ev.cuda_event)) == ref["summary"]
    assert late.potential().tobytes() == ref["P"].tobytes()
    # the field keeps its own copy of the plane: paths do not depend on what becomes of the caller's
    u.fill_(100)
    torch.cuda.synchronize()
    starts = some_starts(rng, w, h, 10)
    cells, lengths = late.paths(starts, 30)
    want_cells, want_lengths = N.paths(geo_of(w, h), ref["costs"], ref["P"], starts, 30)
    assert np.array_equal(lengths, want_lengths) and cells.tobytes() == want_cells.tobytes()
    d_out = C.c_void_p()
    assert lom.capi.lib().lom_navfield_potential_device(late.handle, C.byref(d_out)) == 0 and d_out.value
    torch.cuda.synchronize()


# ---- 5: purity and refusals ----------------------------------------------------------------------------------------------------
def test_two_solves_agree_and_a_refused_call_changes_nothing(lom):
    rng = np.random.default_rng(30)
    w, h = 65, 33
    plane = S.random_plane(rng, w, h)
    goals = border_goals(w, h)
    dev = lom.NavField(RES, ORIGIN, w, h)
    assert (dev.potential() == N.UNREACHED).all()                      # after create
    first = dev.solve(plane, as_tuple(P1), goals)
    a = dev.potential()
    other = S.serpentine(w, h)
    dev.solve(other, as_tuple(P0), goals[:1])
    assert dev.potential().tobytes() != a.tobytes()
    assert dev.solve(plane, as_tuple(P1), goals) == first and dev.potential().tobytes() == a.tobytes()
    ref = reference("purity", w, h, plane, P1, goals)
    assert a.tobytes() == ref["P"].tobytes() and first == ref["summary"]
    starts = some_starts(rng, w, h, 10)
    paths_before = dev.paths(starts, 20)
    L = lom.capi.lib()
    sm = lom.capi.NavFieldSummary()
    g32 = np.ascontiguousarray(goals, np.int32)
    for bad in ((0, 3, 400, 98, 0), (50, 3, 400, 99, 0), (50, 3, 0, 98, 1), (50, 3, 400, 98, 2), (1 << 24, 0, 1, 98, 0)):
        sm.cells_blocked = 9
        prm = lom.navfieldParams(bad)
        assert L.lom_navfield_solve(dev.handle, other.ctypes.data, C.byref(prm), 0, g32.ctypes.data, len(g32), C.byref(sm)) == lom.capi.ERR_ARG
        assert sm.asdict() == dict.fromkeys(N.SUMMARY_KEYS, 0) and L.lom_navfield_last_error(dev.handle)
    good = lom.navfieldParams(as_tuple(P0))
    for args in ((None, C.byref(good), 0, g32.ctypes.data, len(g32)), (other.ctypes.data, None, 0, g32.ctypes.data, len(g32)),
                 (other.ctypes.data, C.byref(good), 2, g32.ctypes.data, len(g32)), (other.ctypes.data, C.byref(good), 0, None, 3),
                 (other.ctypes.data, C.byref(good), 0, g32.ctypes.data, (1 << 24) + 1)):
        sm.cells_blocked = 9
        assert L.lom_navfield_solve(dev.handle, *args, C.byref(sm)) == lom.capi.ERR_ARG
        assert sm.asdict() == dict.fromkeys(N.SUMMARY_KEYS, 0)
    assert L.lom_navfield_solve_device(dev.handle, None, None, C.byref(good), 0, g32.ctypes.data, len(g32), C.byref(sm)) == lom.capi.ERR_ARG
    with pytest.raises(ValueError):
        dev.solve(plane[:-1], as_tuple(P0), goals)
    assert dev.potential().tobytes() == a.tobytes()                    # nothing changed
    after = dev.paths(starts, 20)
    assert after[0].tobytes() == paths_before[0].tobytes() and np.array_equal(after[1], paths_before[1])
    for option, bad in ((lom.capi.NAV_OPT_TEST_INNER_CAP, (1 << 20) + 1), (lom.capi.NAV_OPT_TEST_BATCH, 257),
                        (lom.capi.NAV_OPT_TEST_ALL_TILES, 2), (77, 0)):
        with pytest.raises(lom.LomError):
            dev.setOption(option, bad)
    assert dev.geometry() == dict(resolution=RES, origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=w, height=h)
    assert L.lom_navfield_device(dev.handle) == 0 and L.lom_navfield_stream(dev.handle)
    few = np.full(50, 7, np.uint32)
    assert L.lom_navfield_potential(dev.handle, few.ctypes.data, 20) == 0
    assert np.array_equal(few[:20], a.ravel()[:20]) and (few[20:] == 7).all()
    dev.clear()
    assert (dev.potential() == N.UNREACHED).all() and dev.paths(starts, 5)[1].sum() == 0
    with pytest.raises(lom.LomError) as e:
        lom.NavField(0.5, (0, 0), 10, 8193)
    assert e.value.code == lom.capi.ERR_ARG


# ---- mirrors -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::NavField of the C++ mirror compiles with plain g++ and leaves the bytes the Python package leaves."""
    exe = cpp_program.build_with_library(tmp_path, "test_navfield_mirror.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    lines = stdout.strip().split("\n")
    got_summary = [int(v) for v in lines[-2].split()]
    got_field = np.array([int(v) for v in lines[-1].split()], np.uint64).astype(np.uint32)
    # the same grid, plane and goals here (tests/cpp/test_navfield_mirror.cpp)
    w, h = 45, 37
    i = np.arange(w * h)
    plane = np.where(i % 7 == 3, 100, np.where(i % 5 == 0, -1, (i % 13) * 7)).astype(np.int8).reshape(h, w)
    goals = np.array([(0, 0), (44, 36), (20, 20), (-1, 3), (0, 0)], np.int32)
    p = N.params(20, 2, 300, 80, N.UNKNOWN_PASSABLE)
    dev = lom.NavField(RES, ORIGIN, w, h)
    summary = dev.solve(plane, as_tuple(p), goals)
    field = dev.potential()
    assert got_summary == [summary[k] for k in N.SUMMARY_KEYS]
    assert got_field.tobytes() == field.tobytes()
    ref = N.solve(geo_of(w, h), plane, p, goals)
    assert field.tobytes() == ref["P"].tobytes() and summary == ref["summary"] and summary["cells_reached"] > 500
