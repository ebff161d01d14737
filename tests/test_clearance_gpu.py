"""The clearance grid on the device against tests/clearance_ref.py: the squared distance, the cost, the summary and the
metres as bytes -- all exactly equal.  The distance is an integer; the cost is looked up in the library's own table, which
is compared with the reference's entry by entry (equal or off by one: the last ulp of exp) before it is used."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import elevation_ref as E
from tests import occupancy_ref as O
from tests.test_occupancy_gpu import archive_of
from tests.test_vote_gpu import pose_in_room, room_scan

pytestmark = pytest.mark.gpu

RES = 0.25
RADII = {0: 0.1, 1: 0.3, 2: 0.5, 7: 1.8, 40: 10.0, 254: 63.6}   # R -> an inflation radius at RES that gives it
TABLES = {}


def params_of(R, flags=0):
    p = K.params(RADII[R], min(0.6, RADII[R]), 0.7, flags)
    assert K.radius_cells(p, RES) == R
    return p


def table_of(lom, p, res=RES):
    """the library's table, compared with the reference's once"""
    key = (float(p["inflation_radius"]), float(p["inscribed_radius"]), float(p["decay"]), float(res))
    if key not in TABLES:
        TABLES[key] = lom.clearanceCostTable(p, res)
        K.compare_table(TABLES[key], p, res)
    return TABLES[key]


class Grid:
    """a device grid and the planes the reference expects of it"""

    def __init__(self, lom, w, h, res=RES, origin=(-3.0, 2.0)):
        self.lom, self.geo = lom, K.geometry(res, origin[0], origin[1], w, h)
        self.dev = lom.ClearanceGrid(res, origin, w, h)
        self.state = K.empty_state(self.geo)

    def check_planes(self):
        d2, (cost, summary) = self.dev.distanceSq(), self.dev.cost()
        assert np.array_equal(d2, self.state["d2"]), np.argwhere(d2 != self.state["d2"])[:10]
        assert np.array_equal(cost, self.state["cost"]), np.argwhere(cost != self.state["cost"])[:10]
        assert summary == K.plane_summary(self.state["cost"])
        assert self.dev.distance().tobytes() == K.metres(self.state["d2"], self.geo["resolution"]).tobytes()

    def update(self, occ, elev, p, window=None, metres=True):
        """device and reference, compared: the summary, then d2 and the cost over the whole grid"""
        ref = K.update(self.geo, occ, elev, p, window, self.state, table_of(self.lom, p, self.geo["resolution"]))
        assert not ref["error"]
        summary = self.dev.update(occ, elev, p, window)
        assert summary == ref["summary"], (summary, ref["summary"])
        self.state = dict(d2=ref["d2"], cost=ref["cost"])
        d2 = self.dev.distanceSq()
        assert np.array_equal(d2, ref["d2"]), (window, np.argwhere(d2 != ref["d2"])[:10])
        cost = self.dev.cost()[0]
        assert np.array_equal(cost, ref["cost"]), (window, np.argwhere(cost != ref["cost"])[:10])
        if metres:
            assert self.dev.distance().tobytes() == K.metres(ref["d2"], self.geo["resolution"]).tobytes()
        return ref


def planes(rng, w, h, obstacles):
    """occ: 100 on the obstacles, else 0 or -1; elev: -1 .. 99 at random, so that the cost meets known and unknown bases"""
    occ = rng.choice(np.array([0, -1], np.int8), (h, w))
    occ[obstacles] = 100
    elev = rng.integers(-1, 100, (h, w)).astype(np.int8)
    return occ, elev


def patterns(rng, w, h):
    """name -> bool (h, w)"""
    none = np.zeros((h, w), bool)
    out = dict(none=none, all=~none)
    for name, (y, x) in dict(corner00=(0, 0), corner01=(0, w - 1), corner10=(h - 1, 0), corner11=(h - 1, w - 1)).items():
        out[name] = none.copy()
        out[name][y, x] = True
    out["row"], out["column"] = none.copy(), none.copy()
    out["row"][h // 2, :] = True
    out["column"][:, w // 2] = True
    for x in (0, 63, 64, 127, 128):                                 # bits 0 and 63 of a bitmap word, both sides of a word border
        if x < w:
            out["bit%d" % x] = none.copy()
            out["bit%d" % x][h // 2, x] = True
    for name, share in dict(random_0001=0.001, random_002=0.02, random_05=0.5).items():
        out[name] = rng.random((h, w)) < share
    return out


# ---- 1: shapes x R x obstacle patterns ---------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 200), (200, 1), (45, 37), (63, 3), (64, 3), (65, 3), (130, 67), (257, 40)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_radii_and_patterns(lom, w, h):
    rng = np.random.default_rng(1000 * w + h)
    g = Grid(lom, w, h)
    pats = patterns(rng, w, h)
    if (w, h) == (130, 67):   # what the random cases are for, on the reference first
        assert (K.distance_sq(pats["random_0001"], 7) == K.FAR).any() and pats["random_0001"].any()
        assert not (K.distance_sq(pats["random_05"], 7) == K.FAR).any()
    for name, ob in pats.items():
        occ, elev = planes(rng, w, h, ob)
        for R in RADII:
            ref = g.update(occ, elev, params_of(R), metres=R in (2, 254))
            assert ((ref["d2"] == 0) == (ob | (elev == 100))).all(), (name, R)
    g.check_planes()


def test_large_grid_at_the_largest_radius(lom):
    """1030 x 515 at R = 254: tiles that stage 540 rows, five bitmap words on either side, d2 up to 64516"""
    rng = np.random.default_rng(7)
    w, h = 1030, 515
    g = Grid(lom, w, h)
    ob = np.zeros((h, w), bool)
    ob[rng.integers(0, h, 6), rng.integers(0, w, 6)] = True
    ob[0, 0] = ob[h - 1, w - 1] = True
    occ = np.where(ob, 100, 0).astype(np.int8)
    ref = g.update(occ, None, params_of(254), metres=False)
    near = ref["d2"][ref["d2"] != K.FAR]
    assert near.max() > 250 * 250 and (ref["d2"] == K.FAR).any()
    occ, elev = planes(rng, w, h, rng.random((h, w)) < 0.001)
    g.update(occ, elev, params_of(254))


# ---- 2: purity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,R", [(130, 67, 7), (257, 40, 40), (65, 70, 254)])
def test_bytes_do_not_depend_on_tile_rows_or_pruning(lom, w, h, R):
    rng = np.random.default_rng(R)
    cases = [planes(rng, w, h, rng.random((h, w)) < share) for share in (0.02, 0.0005)]
    for T in (1, 8, 32):
        for no_prune in (0, 1):
            g = Grid(lom, w, h)
            g.dev.setOption(lom.capi.CLEAR_OPT_TEST_TILE_ROWS, T)
            g.dev.setOption(lom.capi.CLEAR_OPT_TEST_NO_PRUNE, no_prune)
            for occ, elev in cases:
                g.update(occ, elev, params_of(R), metres=False)
                g.update(occ, elev, params_of(R), window=(w // 3, h // 4, w // 2, h // 2), metres=False)
    with pytest.raises(lom.LomError):
        g.dev.setOption(lom.capi.CLEAR_OPT_TEST_TILE_ROWS, 33)
    with pytest.raises(lom.LomError):
        g.dev.setOption(lom.capi.CLEAR_OPT_TEST_NO_PRUNE, 2)
    with pytest.raises(lom.LomError):
        g.dev.setOption(77, 0)
    g.dev.setOption(lom.capi.CLEAR_OPT_TEST_TILE_ROWS, -1)
    g.dev.setOption(lom.capi.CLEAR_OPT_TEST_NO_PRUNE, -1)
    g.update(*cases[0], params_of(R), metres=False)


# ---- 3: windows --------------------------------------------------------------------------------------------------------------
WINDOWS = [(0, 0, 1, 1), (256, 69, 1, 1), (60, 30, 10, 5), (63, 31, 2, 2), (-5, -5, 20, 20), (250, 60, 50, 50), (0, 0, 257, 1),
           (128, 0, 1, 70), (10, 3, 100, 50), (64, 0, 64, 32), (1, 1, 255, 68), (-1000, -1000, 5000, 5000)]


@pytest.mark.parametrize("R", [0, 7, 40])
def test_windows_equal_the_full_update_on_their_cells(lom, R):
    rng = np.random.default_rng(40 + R)
    w, h = 257, 70
    g = Grid(lom, w, h)
    before = planes(rng, w, h, rng.random((h, w)) < 0.01)
    after = planes(rng, w, h, rng.random((h, w)) < 0.01)
    p = params_of(R)
    full = K.update(g.geo, *after, p, table=table_of(lom, p))
    for win in WINDOWS:
        g.update(*before, p)                                         # the state every window starts from
        outside = g.state
        ref = g.update(*after, p, window=win)                        # (compares every cell, in the window and outside it)
        x0, y0, x1, y1 = K.clip(win, g.geo)
        assert np.array_equal(ref["d2"][y0:y1, x0:x1], full["d2"][y0:y1, x0:x1])
        assert np.array_equal(ref["cost"][y0:y1, x0:x1], full["cost"][y0:y1, x0:x1])
        mask = np.ones((h, w), bool)
        mask[y0:y1, x0:x1] = False
        assert np.array_equal(ref["d2"][mask], outside["d2"][mask]) and np.array_equal(ref["cost"][mask], outside["cost"][mask])
    # an empty rectangle: LOM_OK, nothing changes, a summary of zeros
    for win in ((257, 0, 5, 5), (0, 70, 5, 5), (-9, 0, 9, 70), (5, 5, 0, 3), (5, 5, 3, 0)):
        assert g.dev.update(*before, p, window=win) == dict.fromkeys(K.SUMMARY_KEYS, 0)
    g.check_planes()
    g.dev.clear()
    g.state = K.empty_state(g.geo)
    g.check_planes()
    g.update(*after, p, window=(100, 20, 30, 30))                    # on a cleared grid: the rest stays far and unknown


def test_an_obstacle_that_moves_under_windowed_updates(lom):
    rng = np.random.default_rng(5)
    w, h, R = 300, 90, 7
    g = Grid(lom, w, h)
    walls = np.zeros((h, w), bool)
    walls[0, :] = walls[-1, :] = True
    p = params_of(R)
    elev = rng.integers(-1, 60, (h, w)).astype(np.int8)
    pos = [(20, 40), (35, 42), (62, 45), (66, 30), (130, 31), (131, 31)]
    for k, (x, y) in enumerate(pos):
        ob = walls.copy()
        ob[y:y + 4, x:x + 6] = True
        occ = np.where(ob, 100, 0).astype(np.int8)
        if k == 0:
            g.update(occ, elev, p)
            continue
        # the rectangle that covers where the mover was and is, grown by R: everything that can change
        px, py = pos[k - 1]
        x0, y0, x1, y1 = min(x, px) - R, min(y, py) - R, max(x, px) + 6 + R, max(y, py) + 4 + R
        ref = g.update(occ, elev, p, window=(x0, y0, x1 - x0, y1 - y0))
        full = K.update(g.geo, occ, elev, p, table=table_of(lom, p))
        assert np.array_equal(ref["d2"], full["d2"]) and np.array_equal(ref["cost"], full["cost"])   # nothing stale is left


# ---- 4: flags, a plane left out, invalid values ---------------------------------------------------------------------------------
def test_flags_planes_left_out_and_invalid_values(lom):
    rng = np.random.default_rng(9)
    w, h = 45, 37
    g = Grid(lom, w, h)
    occ = rng.choice(np.array([-1, 0, 0, 100, 5, -7, 127, -128], np.int8), (h, w))
    elev = rng.choice(np.array([-1, -1, 0, 30, 99, 100, 100, 101, 127, -2, -128], np.int8), (h, w))
    seen = set()
    for flags in range(4):
        for o, e in ((occ, elev), (occ, None), (None, elev)):
            for R in (0, 2, 7):
                ref = g.update(o, e, params_of(R, flags))
                seen.add((ref["summary"]["cells_invalid"] > 0, ref["summary"]["cells_cleared"] > 0))
            g.update(o, e, params_of(2, flags), window=(7, 5, 20, 20))
    assert seen == {(True, True), (True, False)}
    clean_o, clean_e = np.where(np.isin(occ, (-1, 0, 100)), occ, -1).astype(np.int8), np.where((elev >= -1) & (elev <= 100), elev, -1).astype(np.int8)
    ref = g.update(clean_o, clean_e, params_of(2, 3))
    assert ref["summary"]["cells_invalid"] == 0 and ref["summary"]["cells_cleared"] > 0
    # refusals change nothing and zero the summary
    L = lom.capi.lib()
    sm = lom.capi.ClearanceSummary()
    for bad, planes_ in (((1.0, 2.0, 1.0, 0), (occ, elev)), ((64.0, 0.5, 1.0, 0), (occ, elev)), ((1.0, 0.5, np.nan, 0), (occ, elev)),
                         ((1.0, 0.5, 1.0, 8), (occ, elev)), ((1.0, 0.5, 1.0, 0), (None, None))):
        sm.cells_lethal = 9
        prm = lom.clearanceParams(bad)
        args = [None if a is None else a.ctypes.data for a in planes_]
        assert L.lom_clearance_update(g.dev.handle, *args, C.byref(prm), None, C.byref(sm)) == lom.capi.ERR_ARG
        assert sm.asdict() == dict.fromkeys(K.SUMMARY_KEYS, 0) and L.lom_clearance_last_error(g.dev.handle)
        assert L.lom_clearance_update_device(g.dev.handle, None, None, None, C.byref(prm), None, C.byref(sm)) == lom.capi.ERR_ARG
    assert L.lom_clearance_update(g.dev.handle, occ.ctypes.data, None, None, None, None) == lom.capi.ERR_ARG
    with pytest.raises(ValueError):
        g.dev.update(occ[:-1], None, params_of(2))
    g.check_planes()
    assert g.dev.geometry() == dict(resolution=RES, origin_x=-3.0, origin_y=2.0, width=w, height=h)
    assert L.lom_clearance_device(g.dev.handle) == 0 and L.lom_clearance_stream(g.dev.handle)
    # read-back with a cap
    few = np.full(50, 7, np.uint16)
    assert L.lom_clearance_distance_sq(g.dev.handle, few.ctypes.data, 20) == 0
    assert np.array_equal(few[:20], g.state["d2"].ravel()[:20]) and (few[20:] == 7).all()
    with pytest.raises(lom.LomError) as e:
        lom.ClearanceGrid(0.5, (0, 0), 10, 8193)
    assert e.value.code == lom.capi.ERR_ARG


# ---- 5: from the two grids -----------------------------------------------------------------------------------------------------
GEO2 = E.geometry(0.1, -5.0, -4.0, 100, 80, -0.4)  # the room of tests/test_carve_gpu.py (9 x 7 m) and a margin
RAYS = O.ray_params(z_lo=-2.5, z_hi=2.5, margin=0.05, min_range=1.0, max_range=6.0)
POINTS = E.point_params(z_lo=-2.5, z_hi=2.5, min_range=1.0, max_range=6.0)
RULE, LAYER, COST = O.rule(1, 1, 1), E.layer_params(1, 2), E.cost_params(max_slope=2.0, max_step=0.6, max_rough=0.3, max_span=1.5)


def test_update_from_grids(lom):
    rng = np.random.default_rng(92)
    poses = np.stack([pose_in_room(rng, turn=0.6) for _ in range(5)])
    scans = [room_scan(rng, 4000, poses[k])[0] for k in range(5)]
    a = archive_of(lom, scans)
    ids = np.arange(5)
    org = (GEO2["origin_x"], GEO2["origin_y"])
    occ = lom.OccupancyGrid(GEO2["resolution"], org, GEO2["width"], GEO2["height"])
    elev = lom.ElevationGrid(GEO2["resolution"], org, GEO2["width"], GEO2["height"], GEO2["z_ref"])
    occ.integrate(a, ids, poses, RAYS)
    elev.integrate(a, ids, poses, POINTS)
    occ_plane, elev_plane = occ.classify(RULE)[0], elev.cost(LAYER, COST)[0]
    assert (occ_plane == 100).sum() > 100 and (occ_plane == 0).sum() > 1000 and (elev_plane == 100).sum() > 50
    g = Grid(lom, GEO2["width"], GEO2["height"], GEO2["resolution"], org)
    for flags in (0, 1, 3):
        p = K.params(1.0, 0.3, 2.0, flags)
        for o, e in ((occ, elev), (occ, None), (None, elev)):
            for win in (None, (30, 20, 45, 33)):
                ref = K.update(g.geo, None if o is None else occ_plane, None if e is None else elev_plane, p, win, g.state,
                               table_of(lom, p, GEO2["resolution"]))
                got = g.dev.updateFromGrids(o, RULE, e, LAYER, COST, p, win)
                assert got == ref["summary"]
                g.state = dict(d2=ref["d2"], cost=ref["cost"])
                g.check_planes()
        if flags == 1:
            assert ref["summary"]["cells_lethal"] > 0
    # the producers go on: the same planes again, then through the clearance once more
    assert np.array_equal(occ.classify(RULE)[0], occ_plane) and np.array_equal(elev.cost(LAYER, COST)[0], elev_plane)
    # mismatched geometry, bad parameters of any of the three, no grid at all: refused, nothing changes
    p = K.params(1.0, 0.3, 2.0)
    others = [lom.OccupancyGrid(GEO2["resolution"], org, GEO2["width"] + 1, GEO2["height"]),
              lom.OccupancyGrid(GEO2["resolution"], org, GEO2["width"], GEO2["height"] - 1),
              lom.OccupancyGrid(GEO2["resolution"], (org[0] + 1e-6, org[1]), GEO2["width"], GEO2["height"]),
              lom.OccupancyGrid(GEO2["resolution"], (org[0], org[1] - 1e-6), GEO2["width"], GEO2["height"]),
              lom.OccupancyGrid(np.nextafter(GEO2["resolution"], np.float32(1)), org, GEO2["width"], GEO2["height"])]
    refused = [lambda o=o: g.dev.updateFromGrids(o, RULE, elev, LAYER, COST, p) for o in others]
    refused.append(lambda: g.dev.updateFromGrids(occ, RULE, lom.ElevationGrid(GEO2["resolution"], org, 99, 80, 0.0), LAYER, COST, p))
    refused.append(lambda: g.dev.updateFromGrids(occ, O.rule(0, 1, 1), elev, LAYER, COST, p))
    refused.append(lambda: g.dev.updateFromGrids(occ, RULE, elev, E.layer_params(1, 5), COST, p))
    refused.append(lambda: g.dev.updateFromGrids(occ, RULE, elev, LAYER, E.cost_params(0.0, 1, 1, 1), p))
    refused.append(lambda: g.dev.updateFromGrids(occ, RULE, elev, LAYER, COST, K.params(1.0, 2.0, 1.0)))
    refused.append(lambda: g.dev.updateFromGrids(None, RULE, None, LAYER, COST, p))
    if lom.capi.lib().lom_device_count() > 1:
        refused.append(lambda: g.dev.updateFromGrids(lom.OccupancyGrid(GEO2["resolution"], org, GEO2["width"], GEO2["height"], device=1),
                                                     RULE, None, LAYER, COST, p))
    for call in refused:
        with pytest.raises(lom.LomError) as e:
            call()
        assert e.value.code == lom.capi.ERR_ARG
    g.check_planes()


# ---- 6: query ------------------------------------------------------------------------------------------------------------------
def test_query(lom):
    rng = np.random.default_rng(3)
    g = Grid(lom, 45, 37, 0.5, (-4.0, -3.0))                        # x in [-4, 18.5), y in [-3, 15.5)
    occ, elev = planes(rng, 45, 37, rng.random((37, 45)) < 0.03)
    p = K.params(2.6, 0.6, 1.0)
    g.update(occ, elev, p)
    nan, inf = np.nan, np.inf
    xy = [[-4.0, -3.0], [-3.5, -2.5], [-3.5000002, -2.5000002], [18.499998, 15.499999], [18.5, 0.0], [0.0, 15.5],   # cell borders
          [-4.0000005, 0.0], [0.0, -3.0000002], [-4.3, -3.3], [-100.0, 5.0], [5.0, 1e30], [-1e30, -1e30],             # left of, below
          [nan, 0.0], [0.0, nan], [nan, nan], [inf, 0.0], [0.0, -inf], [0.0, 0.0], [0.25, 0.25], [-0.25, -0.25]]
    xy = np.concatenate([np.asarray(xy, np.float32), rng.uniform(-6, 20, (600, 2)).astype(np.float32)])
    dist, cost = g.dev.query(xy)
    want_d, want_c = K.query(g.geo, g.state["d2"], g.state["cost"], xy)
    assert dist.tobytes() == want_d.tobytes() and np.array_equal(cost, want_c)
    assert (want_c[6:17] == -1).all() and np.isnan(want_d[6:17]).all() and not np.isnan(want_d[:4]).any()
    assert np.isinf(want_d).any() and (np.isfinite(want_d) & (want_d > 0)).any()
    d0, c0 = g.dev.query(np.zeros((0, 2), np.float32))
    assert len(d0) == 0 and len(c0) == 0
    L = lom.capi.lib()
    only = np.full(len(xy), 5, np.int8)
    assert L.lom_clearance_query(g.dev.handle, xy.ctypes.data, len(xy), None, only.ctypes.data) == 0 and np.array_equal(only, want_c)
    assert L.lom_clearance_query(g.dev.handle, None, 3, None, only.ctypes.data) == lom.capi.ERR_ARG


# ---- 7: stream order -----------------------------------------------------------------------------------------------------------
def test_device_form_and_a_callers_event(lom):
    import torch

    rng = np.random.default_rng(12)
    w, h = 257, 70
    occ, elev = planes(rng, w, h, rng.random((h, w)) < 0.01)
    p = params_of(7)
    host = Grid(lom, w, h)
    ref = host.update(occ, elev, p)
    # planes in HBM, complete now
    t_occ, t_elev = torch.from_numpy(occ).to("cuda:0"), torch.from_numpy(elev).to("cuda:0")
    torch.cuda.synchronize()
    dev = Grid(lom, w, h)
    got = dev.dev.update(t_occ.data_ptr(), t_elev.data_ptr(), p, device=True)
    assert got == ref["summary"]
    dev.state = host.state
    dev.check_planes()
    got = dev.dev.update(t_occ.data_ptr(), None, p, window=(3, 3, 200, 9), device=True)
    want = K.update(dev.geo, occ, None, p, (3, 3, 200, 9), dev.state, table_of(lom, p))
    assert got == want["summary"]
    dev.state = dict(d2=want["d2"], cost=want["cost"])
    dev.check_planes()
    # planes produced on another stream: the update waits for the caller's event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.ones(1 << 26, device="cuda:0")
        for _ in range(20):                                          # work in front of the planes
            big = big * 1.0001 + 1.0
        u_occ = torch.from_numpy(occ).to("cuda:0", non_blocking=True) + 0
        u_elev = torch.from_numpy(elev).to("cuda:0", non_blocking=True) + 0
        ev = torch.cuda.Event()
        ev.record(s)
    late = Grid(lom, w, h)
    got = late.dev.update(u_occ.data_ptr(), u_elev.data_ptr(), p, device=True, hip_event=C.c_void_p(ev.cuda_event))
    assert got == ref["summary"]
    late.state = host.state
    late.check_planes()
    # cost_device: the plane left in HBM
    d_out = C.c_void_p()
    assert lom.capi.lib().lom_clearance_cost_device(late.dev.handle, C.byref(d_out)) == 0 and d_out.value
    torch.cuda.synchronize()


# ---- mirrors -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::ClearanceGrid of the C++ mirror compiles with plain g++ and leaves what the reference leaves."""
    exe = cpp_program.build_with_library(tmp_path, "test_clearance_mirror.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    got = [int(v) for v in stdout.split()[-8:]]
    # the same grid and planes here (tests/cpp/test_clearance_mirror.cpp)
    i = np.arange(45 * 37)
    occ = np.where(i % 97 == 5, 100, np.where(i % 3 == 0, -1, 0)).astype(np.int8).reshape(37, 45)
    elev = np.where(i % 41 == 7, 100, (i % 11) * 9 - 1).astype(np.int8).reshape(37, 45)
    p = K.params(1.8, 0.6, 0.7, K.FREE_CLEARS_ELEVATION)
    ref = K.update(K.geometry(RES, -3.0, 2.0, 45, 37), occ, elev, p, table=table_of(lom, p))
    assert got[:6] == [ref["summary"][k] for k in K.SUMMARY_KEYS] and ref["summary"]["cells_cleared"] > 0
    assert got[6:] == [int(ref["d2"].astype(np.int64).sum()), int(ref["cost"].astype(np.int64).sum())]
