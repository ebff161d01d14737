"""The visibility grid on the device against tests/visibility_ref.py: the records, the beam words and the windows as bytes,
the summary and the selection's list -- all exactly equal, under every setting of the test switches.  The reference of a
case is computed once (cast_fast, which tests/test_visibility_host.py holds equal to the beam-by-beam form) and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import occupancy_ref as O
from tests import regions_ref as R
from tests import regions_scenes as RS
from tests import visibility_ref as V

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 31), (65, 33), (129, 65)]
# (R, B): 360 and 1000 are no multiples of a workgroup; at R = 31 a window row ends inside a word; at R = 254 the window is
# larger than every grid here
RANGE_BEAMS = [(0, 4), (1, 8), (7, 64), (31, 360), (40, 1000), (254, 2048)]
# (block_min, D), rotated over planes and (R, B) so that each meets all six
MODES = [(100, 0), (50, 1), (100, 5), (50, 0), (100, 1), (50, 5)]
# no LDS, waves
SWITCHES = [(no_lds, waves) for no_lds in (0, 1) for waves in (1, 4)]
KEEP = V.KEEP_WINDOWS | V.KEEP_BEAMS
SELECT = V.select_params(8, 3, 1, 1)
REFS, TABLES = {}, {}


def table_of(lom, beams):
    if beams not in TABLES:
        TABLES[beams] = lom.visibilityTable(beams)
    return TABLES[beams]


def reference(lom, key, plane, vp, p):
    """the reference's cast of a case, once"""
    if key not in REFS:
        REFS[key] = V.cast_fast(plane, vp, table_of(lom, p["beams"]), p)
    return REFS[key]


def set_switches(lom, dev, no_lds, waves):
    dev.setOption(lom.capi.VIS_OPT_TEST_NO_LDS, no_lds)
    dev.setOption(lom.capi.VIS_OPT_TEST_WAVES, waves)


def planes_of(w, h):
    rng = np.random.default_rng(1000 * w + h)
    return {"free": S.empty(w, h), "unknown": np.full((h, w), -1, np.int8), "blocking": RS.full(w, h), "random": S.random_plane(rng, w, h),
            "serpentine": S.serpentine(w, h), "spiral": S.spiral(w, h), "diagonal_gaps": S.diagonal_gaps(w, h), "pocket": S.pocket(w, h),
            "frontier": RS.frontier_plane(w, h)}


def viewpoints_of(plane, rng, extra=5):
    """corners, edge cells, blocking cells, cells outside the grid, a duplicate pair and a few random ones"""
    h, w = plane.shape
    vp = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (0, h // 2), (w - 1, h // 2), (w // 2, h - 1), (w // 2, h // 2), (w // 2, h // 2)]
    vp += [(int(x), int(y)) for y, x in np.argwhere(plane >= 100)[:: max(1, int((plane >= 100).sum()) // 3)][:3]]
    vp += [(-1, 0), (w, 0), (0, h), (0, -1), (w + 5, h + 5), (-300, 2), (1 << 30, -(1 << 30))]
    vp += [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(extra)]
    return np.array(vp, np.int32)


def cost_of(k):
    cost = ((np.arange(k, dtype=np.uint64) * 97) % 1000).astype(np.uint32)
    cost[1::7] = V.UNREACHED
    return cost


def check_cast(dev, ref, plane, vp, p, what=None):
    """one cast against the reference: summary, records, beams, windows, and the launches"""
    summary = dev.cast(plane, vp, V.as_tuple(p))
    assert summary == ref["summary"], (what, summary, ref["summary"])
    got = dev.records()
    assert got.tobytes() == ref["records"].tobytes(), (what, got[:6], ref["records"][:6])
    beams = dev.beams()
    assert beams.tobytes() == ref["beams"].tobytes(), (what, np.argwhere(beams != ref["beams"])[:8])
    windows = dev.windows()
    assert windows.shape == ref["windows"].shape and windows.tobytes() == ref["windows"].tobytes(), (what, np.argwhere(windows != ref["windows"])[:8])
    st = dev.stats()
    assert st == dict(launches=2 if len(vp) else 0, waits=1), (what, st)


def check_select(dev, ref, select, cost, what=None):
    got, want = dev.select(V.select_tuple(select), cost), V.select(ref, select, cost)
    assert got.tobytes() == want.tobytes(), (what, got, want)
    st = dev.stats()
    assert st == dict(launches=1 + 3 * select["n"], waits=1), (what, st)
    return got


# ---- 1: shapes x (R, B) x planes x switches -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_planes_and_switches(lom, w, h):
    rng = np.random.default_rng(w + 7 * h)
    dev = lom.VisibilityGrid(RES, ORIGIN, w, h)
    assert len(dev.records()) == 0 and dev.stats() == dict(launches=0, waits=0)                 # after create
    planes = planes_of(w, h)
    reasons = set()
    for ri, (rng_cells, beams) in enumerate(RANGE_BEAMS):
        for pi, (name, plane) in enumerate(planes.items()):
            block_min, depth = MODES[(ri + pi) % len(MODES)]
            vp = viewpoints_of(plane, rng)
            if name == "random" and rng_cells == 31:                                             # K = 300, some outside the grid
                vp = np.stack([rng.integers(-2, w + 2, 300), rng.integers(-2, h + 2, 300)], axis=1).astype(np.int32)
            p = V.params(beams, rng_cells, block_min, depth, KEEP)
            ref = reference(lom, (w, h, name, rng_cells), plane, vp, p)
            assert not ref["error"]
            reasons |= set(np.unique(ref["beams"] >> 24).tolist())
            for no_lds, waves in SWITCHES:
                set_switches(lom, dev, no_lds, waves)
                check_cast(dev, ref, plane, vp, p, what=(name, rng_cells, beams, block_min, depth, no_lds, waves))
            check_select(dev, ref, SELECT, cost_of(len(vp)), what=(name, rng_cells, beams))
            check_select(dev, ref, V.select_params(3), None, what=(name, rng_cells, beams))
    if w * h > 1000:
        assert reasons == {V.END_INVALID, V.END_EDGE, V.END_RANGE, V.END_HIT, V.END_UNKNOWN, V.END_CORNER}
        r = REFS[(w, h, "random", 31)]["records"]
        assert len(r) == 300 and 0 < (r["valid"] == 0).sum() < 250 and r["unknown"].max() > 10
        assert REFS[(w, h, "blocking", 7)]["summary"]["valid"] == 0 and REFS[(w, h, "unknown", 40)]["summary"]["unknown_max"] > 20


def test_viewpoint_counts_0_1_300(lom):
    w, h = 129, 65
    rng = np.random.default_rng(8)
    plane = RS.frontier_plane(w, h)
    dev = lom.VisibilityGrid(RES, ORIGIN, w, h)
    p = V.params(1000, 40, 100, 0, KEEP)
    for k in (0, 1, 300):
        vp = np.stack([rng.integers(0, w, k), rng.integers(0, h, k)], axis=1).astype(np.int32)
        ref = reference(lom, ("counts", k), plane, vp, p)
        for no_lds, waves in SWITCHES:
            set_switches(lom, dev, no_lds, waves)
            check_cast(dev, ref, plane, vp, p, what=(k, no_lds, waves))
        if k:
            picks = check_select(dev, ref, V.select_params(16, 2, 0, 1), cost_of(k), what=k)
            assert len(picks) == min(16, k) or k == 1
        else:
            assert len(dev.select((16, 1, 0, 1))) == 0 and dev.stats() == dict(launches=0, waits=0)
            assert ref["summary"] == dict.fromkeys(V.SUMMARY_KEYS, 0)
    assert REFS[("counts", 300)]["summary"]["valid"] > 200


# ---- 2: purity and refusals ----------------------------------------------------------------------------------------------------
def test_two_runs_agree_and_a_refused_call_changes_nothing(lom):
    w, h = 129, 65
    rng = np.random.default_rng(30)
    plane = RS.frontier_plane(w, h)
    vp = viewpoints_of(plane, rng, extra=40)
    p = V.params(360, 31, 100, 3, KEEP)
    dev = lom.VisibilityGrid(RES, ORIGIN, w, h)
    first = dev.cast(plane, vp, V.as_tuple(p))
    records, beams, windows, picks = dev.records(), dev.beams(), dev.windows(), dev.select((8, 3, 1, 1), cost_of(len(vp)))
    dev.cast(S.serpentine(w, h), vp[:7], V.as_tuple(V.params(64, 7, 100, 0, KEEP)))
    assert len(dev.records()) == 7
    assert dev.cast(plane, vp, V.as_tuple(p)) == first
    assert dev.records().tobytes() == records.tobytes() and dev.beams().tobytes() == beams.tobytes() and dev.windows().tobytes() == windows.tobytes()
    assert dev.select((8, 3, 1, 1), cost_of(len(vp))).tobytes() == picks.tobytes() and len(picks) == 8
    assert dev.select((8, 3, 1, 1), cost_of(len(vp))).tobytes() == picks.tobytes()             # the covered set starts empty every time
    ref = reference(lom, "purity", plane, vp, p)
    assert first == ref["summary"] and records.tobytes() == ref["records"].tobytes() and picks.tobytes() == V.select(ref, SELECT, cost_of(len(vp))).tobytes()
    # refused: bad values, unknown flag bits, no plane, no viewpoints, too many; the summary is zeroed
    L = lom.capi.lib()
    sm = lom.capi.VisibilitySummary()
    other = S.spiral(w, h)
    for bad in ((3, 31, 100, 0, 0), (8193, 31, 100, 0, 0), (360, 255, 100, 0, 0), (360, 31, 0, 0, 0), (360, 31, 101, 0, 0), (360, 31, -5, 0, 0),
                (360, 31, 100, 65536, 0), (360, 31, 100, 0, 4), (360, 31, 100, 0, 1 << 31)):
        sm.viewpoints = 9
        prm = lom.visibilityParams(bad)
        assert L.lom_visibility_cast(dev.handle, other.ctypes.data, vp.ctypes.data, len(vp), C.byref(prm), C.byref(sm)) == lom.capi.ERR_ARG, bad
        assert sm.asdict() == dict.fromkeys(V.SUMMARY_KEYS, 0) and L.lom_visibility_last_error(dev.handle)
    good = lom.visibilityParams(V.as_tuple(p))
    sm.viewpoints = 9
    assert L.lom_visibility_cast(dev.handle, None, vp.ctypes.data, len(vp), C.byref(good), C.byref(sm)) == lom.capi.ERR_ARG and sm.viewpoints == 0
    assert L.lom_visibility_cast(dev.handle, other.ctypes.data, None, 3, C.byref(good), C.byref(sm)) == lom.capi.ERR_ARG
    assert L.lom_visibility_cast(dev.handle, other.ctypes.data, vp.ctypes.data, (1 << 20) + 1, C.byref(good), C.byref(sm)) == lom.capi.ERR_ARG
    assert L.lom_visibility_cast(dev.handle, other.ctypes.data, vp.ctypes.data, len(vp), None, C.byref(sm)) == lom.capi.ERR_ARG
    assert L.lom_visibility_cast_device(dev.handle, None, None, vp.ctypes.data, len(vp), C.byref(good), C.byref(sm)) == lom.capi.ERR_ARG
    dev.setOption(lom.capi.VIS_OPT_MAX_WINDOW_BYTES, len(vp) * 63 * 2 * 4 - 1)                  # one byte short of these windows
    assert L.lom_visibility_cast(dev.handle, other.ctypes.data, vp.ctypes.data, len(vp), C.byref(good), C.byref(sm)) == lom.capi.ERR_ARG
    assert b"LOM_VIS_OPT_MAX_WINDOW_BYTES" in L.lom_visibility_last_error(dev.handle)
    dev.setOption(lom.capi.VIS_OPT_MAX_WINDOW_BYTES, len(vp) * 63 * 2 * 4)
    assert dev.cast(plane, vp, V.as_tuple(p)) == first
    dev.setOption(lom.capi.VIS_OPT_MAX_WINDOW_BYTES, 0)
    out, n = np.zeros(8, lom.capi.VISIBILITY_PICK), C.c_size_t(5)
    for bad in ((0, 1, 0, 1), (1025, 1, 0, 1), (8, 0, 0, 1), (8, 4097, 0, 1), (8, 1, 32, 1), (8, 1, 0, 0)):
        n.value = 5
        sel = lom.visibilitySelectParams(bad)
        assert L.lom_visibility_select(dev.handle, C.byref(sel), None, out.ctypes.data, C.byref(n)) == lom.capi.ERR_ARG and n.value == 0, bad
    sel = lom.visibilitySelectParams((8, 1, 0, 1))
    assert L.lom_visibility_select(dev.handle, C.byref(sel), None, None, C.byref(n)) == lom.capi.ERR_ARG
    assert L.lom_visibility_select_from_navfield(dev.handle, None, C.byref(sel), out.ctypes.data, C.byref(n)) == lom.capi.ERR_ARG
    with pytest.raises(ValueError):
        dev.cast(plane[:-1], vp, V.as_tuple(p))
    for option, bad in ((lom.capi.VIS_OPT_TEST_NO_LDS, 2), (lom.capi.VIS_OPT_TEST_WAVES, 2), (lom.capi.VIS_OPT_TEST_WAVES, 8), (77, 0)):
        with pytest.raises(lom.LomError):
            dev.setOption(option, bad)
    # nothing changed
    assert dev.records().tobytes() == records.tobytes() and dev.beams().tobytes() == beams.tobytes() and dev.windows().tobytes() == windows.tobytes()
    assert dev.select((8, 3, 1, 1), cost_of(len(vp))).tobytes() == picks.tobytes()
    assert dev.geometry() == dict(resolution=RES, origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=w, height=h)
    assert L.lom_visibility_device(dev.handle) == 0 and L.lom_visibility_stream(dev.handle)
    # a cast that keeps nothing: the records stay, beams, windows and a select are LOM_ERR_STATE
    assert dev.cast(plane, vp, V.as_tuple(dict(p, flags=0))) == first and dev.records().tobytes() == records.tobytes()
    for call in (dev.beams, dev.windows, dev.windowsDevice, lambda: dev.select((8, 3, 1, 1))):
        with pytest.raises(lom.LomError) as e:
            call()
        assert e.value.code == lom.capi.ERR_STATE
    # partial outputs
    few = np.zeros(3, lom.capi.VISIBILITY_RECORD)
    assert L.lom_visibility_records(dev.handle, few.ctypes.data, 3, C.byref(n)) == 0 and n.value == len(vp) and few.tobytes() == records[:3].tobytes()
    dev.clear()
    assert len(dev.records()) == 0
    with pytest.raises(lom.LomError) as e:
        lom.VisibilityGrid(0.5, (0, 0), 10, 8193)
    assert e.value.code == lom.capi.ERR_ARG


# ---- 3: with the other grids -----------------------------------------------------------------------------------------------------
def test_from_occupancy_from_navfield_and_the_regions_goals(lom):
    from tests.test_occupancy_gpu import archive_of
    from tests.test_vote_gpu import pose_in_room, room_scan

    rng = np.random.default_rng(92)
    res, org, w, h = 0.1, (-5.0, -4.0), 100, 80
    poses = np.stack([pose_in_room(rng, turn=0.6) for _ in range(3)])
    scans = [room_scan(rng, 4000, poses[k])[0] for k in range(3)]
    rays = O.ray_params(z_lo=-2.5, z_hi=2.5, margin=0.05, min_range=1.0, max_range=3.0)
    rule = O.rule(1, 1, 1)
    occ = lom.OccupancyGrid(res, org, w, h)
    occ.integrate(archive_of(lom, scans), np.arange(3), poses, rays)
    occ_plane = occ.classify(rule)[0]
    assert (occ_plane == 0).sum() > 500 and (occ_plane == -1).sum() > 500
    # cast_from_occupancy equals cast on the read-back plane, and both the reference
    vp = viewpoints_of(occ_plane, rng, extra=30)
    p = V.params(720, 30, 100, 4, KEEP)
    ref = reference(lom, "occupancy", occ_plane, vp, p)
    dev, host = lom.VisibilityGrid(res, org, w, h), lom.VisibilityGrid(res, org, w, h)
    got = dev.castFromOccupancy(occ, rule, vp, V.as_tuple(p))
    assert got == host.cast(occ_plane, vp, V.as_tuple(p)) == ref["summary"] and got["unknown_total"] > 50
    for a, b, c in ((dev.records(), host.records(), ref["records"]), (dev.beams(), host.beams(), ref["beams"]), (dev.windows(), host.windows(), ref["windows"])):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert dev.stats() == dict(launches=2, waits=1)
    assert np.array_equal(occ.classify(rule)[0], occ_plane)                                      # the producer goes on: the same plane again
    # the chain: the goals of a frontier extract are the viewpoints, a navigation field prices them, a select ranks them --
    # against the references' chain
    plane = RS.frontier_plane(w, h)
    reg = lom.RegionGrid(res, org, w, h)
    rp = R.params(R.FRONTIER, min_cells=3, rank=R.RANK_CELLS)
    reg.extract(plane, R.as_tuple(rp))
    goals = reg.goals(R.GOAL_CENTRE)
    want_goals = R.goals(R.extract(plane, rp)["list"], R.GOAL_CENTRE)
    assert goals.dtype == np.int32 and len(goals) >= 10 and np.array_equal(goals, want_goals)
    ref = reference(lom, "chain", plane, want_goals, p)
    assert dev.cast(plane, goals, V.as_tuple(p)) == ref["summary"] and dev.windows().tobytes() == ref["windows"].tobytes()
    nav = lom.NavField(res, org, w, h)
    nav_params = (50, 3, 400, 98, 1)                                                             # unknown cells are passable, at a price
    robot = np.argwhere(plane == 0)[:1, ::-1].astype(np.int32)
    assert nav.solve(plane, nav_params, robot)["cells_reached"] > 500
    # select_from_navfield equals select with NavField.query's values at the viewpoints' cells
    xy = np.stack([org[0] + (goals[:, 0] + 0.5) * res, org[1] + (goals[:, 1] + 0.5) * res], axis=1).astype(np.float32)
    cost = nav.query(xy)
    want_cost = N.solve(N.geometry(res, org[0], org[1], w, h), plane, N.params(*nav_params), robot)["P"][want_goals[:, 1], want_goals[:, 0]]
    assert np.array_equal(cost, want_cost) and np.array_equal(cost, nav.potential()[goals[:, 1], goals[:, 0]])
    sel = V.select_params(6, 64, 4, 1)
    from_field = dev.selectFromNavfield(nav, V.select_tuple(sel))
    assert dev.stats() == dict(launches=2 + 3 * sel["n"], waits=1)
    with_costs = dev.select(V.select_tuple(sel), cost)
    want = V.select(ref, sel, want_cost)
    assert from_field.tobytes() == with_costs.tobytes() == want.tobytes() and len(want) == 6
    assert (cost[want["k"]] != V.UNREACHED).all() and want.tobytes() != V.select(ref, sel).tobytes()    # the costs matter
    assert np.array_equal(nav.potential()[goals[:, 1], goals[:, 0]], cost)                       # the field goes on
    # a differing geometry is refused before any launch, and nothing changes
    before = dev.records()
    refused = [lambda: dev.castFromOccupancy(lom.OccupancyGrid(res, org, w + 1, h), rule, vp, V.as_tuple(p)),
               lambda: dev.castFromOccupancy(occ, O.rule(0, 1, 1), vp, V.as_tuple(p)),
               lambda: dev.selectFromNavfield(lom.NavField(res, (org[0] + 1e-6, org[1]), w, h), V.select_tuple(sel))]
    for call in refused:
        with pytest.raises(lom.LomError) as e:
            call()
        assert e.value.code == lom.capi.ERR_ARG
    assert dev.records().tobytes() == before.tobytes() and dev.select(V.select_tuple(sel), cost).tobytes() == want.tobytes()


def test_device_form_and_a_callers_event(lom):
    import torch

    w, h = 129, 65
    rng = np.random.default_rng(12)
    plane = RS.frontier_plane(w, h)
    vp = viewpoints_of(plane, rng, extra=20)
    p = V.params(360, 31, 100, 2, KEEP)
    ref = reference(lom, "device_form", plane, vp, p)
    dev = lom.VisibilityGrid(RES, ORIGIN, w, h)
    t = torch.from_numpy(plane).to("cuda:0")
    torch.cuda.synchronize()
    assert dev.cast(t.data_ptr(), vp, V.as_tuple(p), device=True) == ref["summary"]
    assert dev.records().tobytes() == ref["records"].tobytes() and dev.windows().tobytes() == ref["windows"].tobytes()
    t.zero_()                                                          # the handle keeps its own copy of the plane
    torch.cuda.synchronize()
    # a plane produced on another stream: the cast waits for the caller's event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.ones(1 << 24, device="cuda:0")
        for _ in range(10):                                           # work in front of the plane
            big = big * 1.0001 + 1.0
        t2 = torch.from_numpy(plane).to("cuda:0", non_blocking=True) + 0
        ev = torch.cuda.Event()
        ev.record(s)
    late = lom.VisibilityGrid(RES, ORIGIN, w, h)
    assert late.cast(t2.data_ptr(), vp, V.as_tuple(p), device=True, hip_event=C.c_void_p(ev.cuda_event)) == ref["summary"]
    assert late.records().tobytes() == ref["records"].tobytes() and late.beams().tobytes() == ref["beams"].tobytes()
    d, words = late.windowsDevice()
    assert d and words == 63 * 2
    torch.cuda.synchronize()


# ---- mirrors -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::VisibilityGrid of the C++ mirror compiles with plain g++ and leaves the bytes the Python package leaves."""
    exe = cpp_program.build_with_library(tmp_path, "test_visibility_mirror.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    lines = stdout.rstrip("\n").split("\n")
    got_summary = [int(v) for v in lines[-5].split()]
    got_records = np.array([int(v) for v in lines[-4].split()], np.int64).reshape(-1, 8)
    got_beams = np.array([int(v) for v in lines[-3].split()], np.uint64).astype(np.uint32)
    got_windows = np.array([int(v) for v in lines[-2].split()], np.uint64).astype(np.uint32)
    got_picks = np.array([int(v) for v in lines[-1].split()], np.int64).reshape(-1, 3)
    # the same grid, plane and viewpoints here (tests/cpp/test_visibility_mirror.cpp)
    w, h = 45, 37
    i = np.arange(w * h)
    plane = np.where(i % 7 == 3, 100, np.where((i % 5 == 0) | (i % 11 == 2), -1, 0)).astype(np.int8).reshape(h, w)
    vp = np.array([[(k * 13) % 50 - 2, (k * 7) % 40 - 1] for k in range(12)], np.int32)
    p = V.params(90, 9, 100, 2, KEEP)
    dev = lom.VisibilityGrid(RES, ORIGIN, w, h)
    summary = dev.cast(plane, vp, V.as_tuple(p))
    cost = ((np.arange(12) * 5) % 7).astype(np.uint32)
    picks = dev.select((4, 2, 0, 1), cost)
    assert got_summary == [summary[k] for k in V.SUMMARY_KEYS]
    assert got_records.tolist() == [[int(v) for v in r] for r in dev.records()]
    assert got_beams.tobytes() == dev.beams().tobytes() and got_windows.tobytes() == dev.windows().tobytes()
    assert got_picks.tolist() == [[int(v) for v in e] for e in picks]
    ref = V.cast_fast(plane, vp, table_of(lom, 90), p)
    assert summary == ref["summary"] and dev.records().tobytes() == ref["records"].tobytes()
    assert picks.tobytes() == V.select(ref, V.select_params(4, 2, 0, 1), cost).tobytes() and len(picks) == 4 and 0 < summary["valid"] < 12
