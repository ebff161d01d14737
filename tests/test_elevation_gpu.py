"""The elevation grid on the device against tests/elevation_ref.py: the four accumulators of every cell, every stats
field, the six layers as bytes, the cost and its summary -- all exactly equal: the accumulators are integers and every f64
operation of the layers is rounded on its own, so there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import cpp_program
from tests import elevation_ref as E
from tests import occupancy_ref as O
from tests.test_occupancy_gpu import archive_of
from tests.test_vote_gpu import pose_in_room, room_scan

pytestmark = pytest.mark.gpu

Q = E.Q
EMPTY = E.I32_MAX  # in a table of heights: no point in this cell


class Grid:
    """a device grid and the cells the reference expects of it"""

    def __init__(self, lom, geo, merge=None):
        self.lom, self.geo = lom, geo
        self.dev = lom.ElevationGrid(geo["resolution"], (geo["origin_x"], geo["origin_y"]), geo["width"], geo["height"], geo["z_ref"])
        self.cells = E.empty_cells(geo)
        if merge is not None:
            self.dev.setOption(lom.capi.ELEV_OPT_TEST_WAVE_MERGE, merge)

    def check_cells(self, cells=None):
        want = self.cells if cells is None else cells
        got = dict(zip(("count", "zmin", "zmax", "sum"), self.dev.cells()))
        for k in ("count", "zmin", "zmax", "sum"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:10])

    def integrate(self, archive, scans, ids, poses, p):
        """device and reference, compared: stats, then the cells"""
        ref = E.integrate(self.geo, scans, ids, poses, p, self.cells)
        assert not ref["error"]
        st = self.dev.integrate(archive, ids, poses, p)
        assert st == ref["stats"], (st, ref["stats"])
        self.cells = ref["cells"]
        self.check_cells()
        return ref

    def check_layers(self, lp):
        got, want = self.dev.layers(lp), E.layers(self.geo, self.cells, lp)
        for k in E.LAYERS:
            assert got[k].tobytes() == want[k].tobytes(), (k, lp, np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))[:10])
        return want

    def check_cost(self, lp, cp):
        cost, summary = self.dev.cost(lp, cp)
        want, want_summary, seen = E.cost(self.geo, self.cells, lp, cp)
        assert np.array_equal(cost, want), np.argwhere(cost != want)[:10]
        assert summary == want_summary
        return want, want_summary, seen

    def clear(self):
        self.dev.clear()
        self.cells = E.empty_cells(self.geo)
        self.check_cells()


# ---- 1: hand-written points ------------------------------------------------------------------------------------------------
GEO1 = E.geometry(0.5, -4.0, -3.0, 45, 37, 0.25)  # x in [-4, 18.5), y in [-3, 15.5); the width is no multiple of 32
P1 = E.point_params(z_lo=-1.0, z_hi=0.5, min_range=1.0, max_range=6.0)
P_WIDE = E.point_params(z_lo=-5000.0, z_hi=5000.0, min_range=0.5, max_range=5000.0)
nan, inf = np.nan, np.inf
U = 2.0 ** -12  # an f32 ulp at 2048
HAND = [  # (origin, endpoints relative to it, parameters): the identity rotation, so the sensor frame is the map's, moved
    ((2.25, 2.25, 1.0), [
        [1.75, 0, 0], [1.75, 1.75, 0], [-1.75, 0.25, 0], [2.0, -2.25, 0.1],     # on cell borders (x = 4, y = 4, x = 0.5, y = 0)
        [3, 1, 0.5], [3, 1, 0.75], [3, 1, -1.0], [3, 1, -1.25],                   # both band edges, and just outside
        [1, 0, 0], [0.75, 0, 0], [6, 0, 0], [6.5, 0, 0],                          # L == min_range, below; L == max_range, beyond
        [0, 0, 0], [nan, 0, 0], [inf, 1, 0], [0, -inf, 0], [1, 1, nan], [1, 1, inf], [1, 1, -inf],
    ], P1),
    ((-3.0, -2.0, 0.5), [[-1.0, 0.3, 0], [-1.25, 0.3, 0], [0.3, -1.0, 0], [0.3, -1.25, 0],   # the grid's own border; left of and
                         [-1.25, -1.25, 0], [1.1, 1.1, -0.5]], P1),                           # below the origin: floor, not truncation
    ((17.5, 14.5, 0.0), [[0.9, 0.9, 0.2], [1.0, 0, 0.2], [0, 1.0, 0.2], [-1.0, -1.0, 0.3], [1.2, 0, 0]], P1),   # the far corner
    ((3.0, 3.0, 0.0), [                                                           # h at +-2048 and just inside (z_ref = 0.25)
        [1, 1, 2048.25], [1, 1, 2048.25 - U], [1, 1, -2047.75], [1, 1, -2047.75 + U], [1, 2, 2300.0], [1, 2, -2300.0],
        [2, 1, 0.25 + 0.5 * Q], [2, 1, 0.25 + 1.5 * Q], [2, 1, 0.25 + 2.5 * Q],   # h * 256 exactly on .5: ties to even
        [2, 2, 0.25 - 0.5 * Q], [2, 2, 0.25 - 1.5 * Q], [2, 2, 0.25 - 2.5 * Q], [2, 3, 0.25 + 100.5 * Q], [2, 3, 0.25 - 101.5 * Q],
    ], P_WIDE),
    ((5.0, 5.0, 0.3), [[2.1 + 0.001 * k, 1.1, 0.01 * (k % 37) - 0.2] for k in range(300)], P1),   # 300 points in a row, one cell
    ((5.0, 5.0, 0.3), [[2.1 + 0.5 * (k & 1), 1.3, 0.004 * k - 0.3] for k in range(128)], P1),     # two cells, lane by lane
    ((5.2, 5.1, 0.1), [[1.9, 1.1, -0.7]], P1),                                                    # n = 1; the same cell again
    ((4.0, 9.0, 0.2), [[1.5 + 0.01 * k, 0.02 * k - 2.0, 0.003 * k - 0.4] for k in range(257)], P1),   # n = 257: a second block
    ((4.0, 9.0, 0.2), [], P1),                                                                    # an empty scan
]


@pytest.mark.parametrize("merge", [1, 0])
def test_hand_written_points(lom, merge):
    scans = [np.asarray(pts, np.float32).reshape(-1, 3) for _, pts, _ in HAND]
    poses = np.array([[*o, 1, 0, 0, 0] for o, _, _ in HAND], np.float64)
    a = archive_of(lom, scans)
    g = Grid(lom, GEO1, merge)
    marked, out_of_height = [], []
    for k, (_, _, p) in enumerate(HAND):  # every scan on its own, on top of each other
        ref = g.integrate(a, scans, [k], poses[k:k + 1], p)
        marked.append(ref["stats"]["points_marked"])
        out_of_height.append(ref["stats"]["points_out_of_height"])
    # what the cases are for, on the reference: the band and the range, the borders, the height limit, the ties
    assert marked == [8, 3, 2, 10, 300, 128, 1, 257, 0] and out_of_height == [0, 0, 0, 4, 0, 0, 0, 0, 0]
    c = g.cells
    assert c["count"][14, 16] == 3 and c["count"][13, 16] == 0 and c["count"][10, 16] == 1   # x = 4, y = 4 exactly: the upper cell
    assert c["count"][2, 0] == 1 and c["count"][0, 2] == 1 and c["count"][36, 44] == 1 and c["count"][:, 0].sum() == 1
    assert (c["zmin"][14, 16], c["zmax"][14, 16]) == (-2 ** 19, 2 ** 19)             # |zq| <= 2^19 is reached
    assert (c["zmin"][14, 18], c["zmax"][14, 18], c["sum"][14, 18]) == (0, 2, 4)     # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert (c["zmin"][16, 18], c["zmax"][16, 18], c["sum"][16, 18]) == (-2, 0, -4)
    assert (c["zmin"][18, 18], c["zmax"][18, 18]) == (-102, 100)
    assert c["count"][18, 22] == 300 + 64 + 1 and c["count"][18, 23] == 64          # the same cell from three scans
    # all of the first group again in one call, twice over: an id given twice counts twice
    ids = [0, 1, 2, 4, 5, 6, 7, 8, 4]
    ref = g.integrate(a, scans, ids, poses[ids], P1)
    assert ref["stats"]["cells_new"] == 0 and ref["cells"]["count"][18, 22] == 2 * 365 + 300
    g.check_layers(E.layer_params(1, 1))
    g.check_cost(E.layer_params(1, 2), E.cost_params(0.3, 0.2, 0.05, 1.0))


def test_far_translation_rounds_the_pose_once(lom):
    """the origin is the pose's translation rounded to f32, the endpoint the f64 transform rounded once: a pose far from
    zero, where the two differ in their last bits"""
    geo = E.geometry(0.5, 100000.0, -50005.0, 45, 37, 2.0)
    pose = np.array([100003.123456789, -50002.987654321, 1.23456789, 0.9, 0.05, -0.03, 0.4])
    assert np.float32(pose[0]) != pose[0] and np.float32(pose[1]) != pose[1]
    rng = np.random.default_rng(5)
    pts = (rng.uniform(-1, 1, (700, 3)) * [6.0, 6.0, 1.0]).astype(np.float32)
    a = archive_of(lom, [pts])
    g = Grid(lom, geo)
    ref = g.integrate(a, [pts], [0], pose[None], E.point_params(-1.0, 1.0, 0.5, 5.5))
    assert 150 < ref["stats"]["points_marked"] < 700
    g.check_layers(E.layer_params(2, 2))


# ---- 2: room scans ---------------------------------------------------------------------------------------------------------
GEO2 = E.geometry(0.1, -5.0, -4.0, 100, 80, -0.4)  # the room of tests/test_carve_gpu.py (9 x 7 m) and a margin
P2 = E.point_params(z_lo=-2.5, z_hi=2.5, min_range=1.0, max_range=6.0)


@pytest.fixture(scope="module")
def room():
    """65 scans of about 4,000 points, poses rotated, quaternions not normalised; id 7 is given twice, with two poses.  The
    reference of the first 1, 7 and 65 and of all 66, computed once and left unchanged"""
    rng = np.random.default_rng(92)
    sizes = rng.integers(3900, 4101, 65)
    poses = np.stack([pose_in_room(rng, turn=0.6) for _ in range(66)])
    scans = [room_scan(rng, int(n), poses[k])[0] for k, n in enumerate(sizes)]
    ids = np.r_[np.arange(65), 7]
    refs = {}
    for K in (1, 7, 65, 66):
        refs[K] = E.integrate(GEO2, scans, ids[:K], poses[:K], P2)
        assert not refs[K]["error"]
        for v in refs[K]["cells"].values():
            v.setflags(write=False)
    assert refs[66]["cells"]["count"].max() > 200 and 0 < refs[1]["stats"]["points_marked"] < sizes[0]
    return scans, ids, poses, refs


@pytest.fixture(scope="module")
def room_archive(lom, room):
    return archive_of(lom, room[0])


@pytest.mark.parametrize("K", [1, 7, 65, 66])
def test_room_scans_with_and_without_the_wave_merge(lom, room, room_archive, K):
    scans, ids, poses, refs = room
    ref = refs[K]
    for merge in (1, 0, -1):
        g = Grid(lom, GEO2, merge)
        st = g.dev.integrate(room_archive, ids[:K], poses[:K], P2)
        assert st == ref["stats"]
        g.check_cells(ref["cells"])


def test_two_calls_equal_one_and_clear(lom, room, room_archive):
    scans, ids, poses, refs = room
    g = Grid(lom, GEO2)
    first = g.integrate(room_archive, scans, ids[:3], poses[:3], P2)
    second = g.integrate(room_archive, scans, ids[3:7], poses[3:7], P2)                  # on top of the first
    g.check_cells(refs[7]["cells"])
    assert first["stats"]["cells_new"] + second["stats"]["cells_new"] == refs[7]["stats"]["cells_new"]
    g.clear()                                                                             # every cell empty again
    cost, summary = g.dev.cost(E.layer_params(1, 1), E.cost_params(1, 1, 1, 1))
    assert (cost == -1).all() and summary == dict(cells_unknown=8000, cells_lethal=0, cells_costed=0)
    assert np.isnan(g.dev.layers(E.layer_params(1, 1))["min"]).all()
    st = g.dev.integrate(room_archive, [7, 7], poses[[7, 65]], P2)                          # an id twice counts twice
    want = E.integrate(GEO2, scans, [7, 7], poses[[7, 65]], P2)
    assert st == want["stats"]
    g.check_cells(want["cells"])
    st = g.dev.integrate(room_archive, [], np.empty((0, 7)), P2)                            # nothing to do
    assert st == dict(scans=0, points=0, points_marked=0, points_out_of_height=0, cells_new=0)
    g.check_cells(want["cells"])


def test_count_equals_the_occupancy_grids_seen(lom, room, room_archive):
    """the library against itself: a cell has points iff some scan hit it in a lom_occupancy grid of the same geometry,
    scans and parameters (no point of the room is out of the height range)"""
    scans, ids, poses, refs = room
    assert refs[7]["stats"]["points_out_of_height"] == 0
    occ = lom.OccupancyGrid(GEO2["resolution"], (GEO2["origin_x"], GEO2["origin_y"]), GEO2["width"], GEO2["height"])
    st = occ.integrate(room_archive, ids[:7], poses[:7], O.ray_params(P2["z_lo"], P2["z_hi"], 0.05, P2["min_range"], P2["max_range"]))
    _, seen = occ.counts()
    g = Grid(lom, GEO2)
    est = g.dev.integrate(room_archive, ids[:7], poses[:7], P2)
    count = g.dev.cells()[0]
    assert np.array_equal(count > 0, seen > 0) and (seen > 0).sum() > 1000
    assert est["points_marked"] == st["endpoints_marked"] == count.sum()


# ---- 3: layers and cost ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("min_points", [1, 3])
def test_layers_and_cost_of_the_room(lom, room, room_archive, R, min_points):
    scans, ids, poses, refs = room
    g = Grid(lom, GEO2)
    g.dev.integrate(room_archive, ids[:7], poses[:7], P2)
    g.cells = refs[7]["cells"]
    lp = E.layer_params(min_points, R)
    want = g.check_layers(lp)
    valid = ~np.isnan(want["min"])
    assert 1000 < valid.sum() < 8000 and np.isfinite(want["slope"]).sum() > 800
    _, summary, seen = g.check_cost(lp, E.cost_params(max_slope=2.0, max_step=0.6, max_rough=0.3, max_span=1.5))
    assert summary["cells_lethal"] > 50 and summary["cells_costed"] > 50 and summary["cells_unknown"] == (~valid).sum()


def heights_to_cloud(geo, z):
    """points at the cell centres of the table z (quanta relative to z_ref; EMPTY: none), three per cell: at z, z + 5 and
    z + 2 quanta -- so zmin = z, span = 5 quanta, count = 3"""
    z = np.asarray(z, np.int64)
    iy, ix = np.nonzero(z != EMPTY)
    x = geo["origin_x"] + (ix + 0.5) * geo["resolution"]
    y = geo["origin_y"] + (iy + 0.5) * geo["resolution"]
    pts = [np.stack([x, y, geo["z_ref"] + (z[iy, ix] + dz) * Q], 1) for dz in (0, 5, 2)]
    return np.concatenate(pts).astype(np.float32)


def grid_from_heights(lom, geo, z, extra=None):
    """a Grid whose cells hold the table (heights_to_cloud) and the points `extra`, seen from outside the grid"""
    pts = heights_to_cloud(geo, z)
    if extra is not None:
        pts = np.concatenate([pts, np.asarray(extra, np.float32).reshape(-1, 3)])
    pose = np.array([geo["origin_x"] - 3.0, geo["origin_y"] - 3.0, geo["z_ref"], 1, 0, 0, 0], np.float64)
    sensor = (pts.astype(np.float64) - pose[:3]).astype(np.float32)   # (exact: halves and quarters)
    a = archive_of(lom, [sensor])
    g = Grid(lom, geo)
    g.integrate(a, [sensor], [0], pose[None], E.point_params(-100.0, 100.0, 0.5, 200.0))
    have = np.asarray(z) != EMPTY
    assert np.array_equal(g.cells["count"] > 0, have | (g.cells["count"] > 3)) and (g.cells["zmin"][have] <= np.asarray(z)[have]).all()
    return g


def test_plane_line_and_single_cell(lom):
    """an exact plane (slope 13 / 128 everywhere, the edges included, roughness 0), a single row and an isolated cell
    (det == 0: NaN slope and roughness, the step still there), on a grid whose tile is cut on both axes"""
    geo = E.geometry(0.5, -2.0, 1.0, 37, 19, 1.0)
    X, Y = np.meshgrid(np.arange(37), np.arange(19))
    g = grid_from_heights(lom, geo, 12 * X - 5 * Y + 40)
    for R in (1, 2, 4):
        want = g.check_layers(E.layer_params(3, R))
        assert (want["slope"] == np.float32(13.0 / 128.0)).all() and (want["rough"] == 0).all()
    assert np.isnan(g.check_layers(E.layer_params(4, 2))["min"]).all()     # min_points above every count
    z = np.full((19, 37), EMPTY, np.int64)
    z[3, :] = 10 * np.arange(37)
    z[9, 35] = 77
    z[17:19, 0:2] = [[1, 2], [3, 5]]
    g = grid_from_heights(lom, geo, z)
    for R in (1, 2, 4):
        want = g.check_layers(E.layer_params(1, R))
        assert np.isnan(want["slope"][3]).all() and np.isnan(want["rough"][9, 35]) and want["step"][9, 35] == 0
        assert np.isfinite(want["slope"][17:19, 0:2]).all() and want["step"][3, 5] == np.float32(10 * Q)
        _, summary, seen = g.check_cost(E.layer_params(1, R), E.cost_params(1.0, 0.05, 1.0, 1.0))
        assert seen["flat_fit"].sum() == 38 and summary["cells_costed"] >= 38


@pytest.mark.parametrize("R", [1, 2, 4])
def test_a_grid_narrower_than_the_window(lom, R):
    geo = E.geometry(0.25, 0.0, 0.0, 3, 40, -1.0)
    rng = np.random.default_rng(17)
    z = rng.integers(-60, 60, (40, 3))
    z[rng.random((40, 3)) < 0.15] = EMPTY
    g = grid_from_heights(lom, geo, z)
    want = g.check_layers(E.layer_params(2, R))
    assert np.isfinite(want["slope"]).sum() > 80
    g.check_cost(E.layer_params(2, R), E.cost_params(1.5, 0.2, 0.1, 0.5))


def test_cost_lands_on_every_branch(lom):
    geo = E.geometry(1.0, 0.0, 0.0, 12, 5, 0.0)
    z = np.zeros((5, 12), np.int64)
    z[:, 4:] = 64          # a step of exactly 0.25 m between columns 3 and 4: m == 1
    z[:, 8:] = 64 + 80     # one of 0.3125 m between columns 7 and 8: lethal
    z[0, 0] = EMPTY
    g = grid_from_heights(lom, geo, z, extra=[[1.5, 2.5, 300 * Q]])          # and a span of 300 quanta in cell (1, 2)
    want, summary, seen = g.check_cost(E.layer_params(1, 1), E.cost_params(max_slope=10.0, max_step=0.25, max_rough=10.0, max_span=1.0))
    assert want[0, 0] == -1 and want[2, 1] == 100 and want[2, 3] == 99 and want[2, 4] == 99 and want[2, 10] == 0
    assert seen["m_is_one"][2, 3] and seen["lethal_step"][2, 7] and seen["lethal_span"][2, 1] and not seen["lethal_slope"].any()
    assert summary["cells_unknown"] == 1 and summary["cells_lethal"] == (want == 100).sum()
    X, Y = np.meshgrid(np.arange(12), np.arange(5))
    g = grid_from_heights(lom, geo, 100 * X)                                 # slope 0.390625
    want, _, seen = g.check_cost(E.layer_params(1, 2), E.cost_params(0.3, 1.0, 1.0, 1.0))
    assert (want == 100).all() and seen["lethal_slope"].all() and not seen["lethal_step"].any()
    want, _, _ = g.check_cost(E.layer_params(1, 2), E.cost_params(0.78125, 1.0, 1.0, 1.0))
    assert (want == 49).all()
    g = grid_from_heights(lom, geo, 40 * ((X + Y) % 2))
    want, _, seen = g.check_cost(E.layer_params(1, 2), E.cost_params(1.0, 1.0, 0.01, 1.0))
    assert seen["m_above_one"].all() and (want == 99).all()
    # cost_device: the same bytes left in HBM (the summary through the host form)
    d_out = C.c_void_p()
    lp, cp = lom.elevationLayerParams((1, 2)), lom.elevationCostParams((1.0, 1.0, 0.01, 1.0))
    assert lom.capi.lib().lom_elevation_cost_device(g.dev.handle, C.byref(lp), C.byref(cp), C.byref(d_out)) == 0 and d_out.value


# ---- 4: the cloud forms ----------------------------------------------------------------------------------------------------
def test_cloud_forms_equal_the_archive_form(lom, room):
    L = lom.capi.lib()
    scans, ids, poses, _ = room
    x, pose = scans[3], poses[3]
    a = lom.ScanArchive()
    assert a.addPoints(x) == 0
    want = Grid(lom, GEO2)
    ref = want.integrate(a, [x], [0], pose[None], P2)
    prm, gp = lom.elevationPointParams(P2), np.zeros(1, lom.capi.GRAPH_POSE)
    gp["t"][0], gp["q_wxyz"][0] = pose[:3], pose[3:]
    ws, dx, dn = lom.VoxelGrid(0.5, 1), C.c_void_p(), C.c_void_p()        # clouds in HBM: another handle's staging buffers
    for stride in (12, 16, 32):
        rec = np.full((len(x), stride // 4), 7.0, np.float32)             # records that begin with x, y, z
        rec[:, :3] = x
        for where in ("host", "device"):
            g = Grid(lom, GEO2)
            st = lom.capi.ElevationStats()
            if where == "host":
                rc = L.lom_elevation_integrate_cloud(g.dev.handle, rec.ctypes.data, len(rec), stride, gp.ctypes.data, C.byref(prm), C.byref(st))
                assert rc == 0 and st.asdict() == ref["stats"]
            else:
                lom.capi.check(L.lom_upload_points(ws.handle, rec.ctypes.data, rec.ctypes.data, len(rec), stride, C.byref(dx), C.byref(dn)), ws.handle)
                lom.capi.check(L.lom_map_status(ws.handle), ws.handle)     # (waits for that handle's copies)
                assert g.dev.integrateCloud(None, pose, P2, device_ptr=dx, n=len(rec), stride_bytes=stride) == ref["stats"]
            g.check_cells(ref["cells"])
    g = Grid(lom, GEO2)
    assert g.dev.integrateCloud(x, pose, P2) == ref["stats"]               # the mirror's host form
    g.check_cells(ref["cells"])
    assert g.dev.integrateCloud(np.zeros((0, 3), np.float32), pose, P2)["points"] == 0   # n == 0: LOM_OK, nothing changes
    g.check_cells(ref["cells"])


# ---- 5: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_cells_unchanged(lom, room):
    L = lom.capi.lib()
    scans, ids, poses, _ = room
    a = archive_of(lom, scans[:3])
    g = Grid(lom, GEO2)
    g.integrate(a, scans, [0, 1, 2], poses[:3], P2)
    zero = lom.capi.ElevationStats().asdict()

    def refused(code, ids_, poses_, prm=P2):
        ids64, gp = np.ascontiguousarray(ids_, np.int64), np.zeros(len(ids_), lom.capi.GRAPH_POSE)
        pp = np.asarray(poses_, np.float64).reshape(-1, 7)
        gp["t"], gp["q_wxyz"] = pp[:, :3], pp[:, 3:]
        st, p = lom.capi.ElevationStats(), lom.elevationPointParams(prm)
        st.scans = 9
        assert L.lom_elevation_integrate(g.dev.handle, a.handle, ids64.ctypes.data, gp.ctypes.data, len(ids64), C.byref(p),
                                         C.byref(st)) == code, (ids_, prm)
        assert st.asdict() == zero and L.lom_elevation_last_error(g.dev.handle)
        x = np.ascontiguousarray(scans[0])
        if len(ids64) == 1 and ids64[0] == 0:  # the cloud form refuses the same pose and parameters
            assert L.lom_elevation_integrate_cloud(g.dev.handle, x.ctypes.data, len(x), 12, gp.ctypes.data, C.byref(p), C.byref(st)) == code
        g.check_cells()

    for change in (dict(z_lo=0.0), dict(z_lo=0.2), dict(z_hi=0.0), dict(z_hi=np.inf), dict(min_range=0.0), dict(min_range=np.nan),
                   dict(max_range=0.2), dict(max_range=np.inf), dict(max_range=0.1 * 2.0 ** 20 * 1.01)):
        refused(lom.capi.ERR_ARG, [0], poses[:1], dict(P2, **change))
    for ids_, p in (([3], poses[:1]), ([-1], poses[:1]), ([0], [[0, 0, 0, 0, 0, 0, 0.0]]), ([0, 1], [poses[0], [np.nan, 0, 0, 1, 0, 0, 0]])):
        refused(lom.capi.ERR_ARG, ids_, p)
    refused(lom.capi.ERR_RANGE, [0], [[0.1 * 2.0 ** 30 * 1.01, 0, 0, 1, 0, 0, 0]])     # an origin cell beyond 2^30
    refused(lom.capi.ERR_RANGE, [1, 0], [poses[1], [0, -1e300, 0, 1, 0, 0, 0]])         # rounds to -inf in f32
    assert E.integrate(GEO2, scans, [1, 0], [poses[1], [0, -1e300, 0, 1, 0, 0, 0]], P2)["error"]
    g.dev.integrate(a, [0], [[0.1 * 2.0 ** 30 * 0.9, 0, 0, 1, 0, 0, 0]], P2)            # inside the range, far from the grid: legal
    g.check_cells()
    x = np.ascontiguousarray(scans[0])
    gp, p = np.zeros(1, lom.capi.GRAPH_POSE), lom.elevationPointParams(P2)
    gp["q_wxyz"][0, 0] = 1.0
    for stride in (8, 14):
        assert L.lom_elevation_integrate_cloud(g.dev.handle, x.ctypes.data, len(x), stride, gp.ctypes.data, C.byref(p), None) == lom.capi.ERR_ARG
    assert L.lom_elevation_integrate_cloud(g.dev.handle, None, len(x), 12, gp.ctypes.data, C.byref(p), None) == lom.capi.ERR_ARG
    assert L.lom_elevation_integrate_cloud(g.dev.handle, x.ctypes.data, len(x), 12, None, C.byref(p), None) == lom.capi.ERR_ARG
    assert L.lom_elevation_integrate_cloud_device(g.dev.handle, None, len(x), 12, gp.ctypes.data, C.byref(p), None, None) == lom.capi.ERR_ARG
    assert L.lom_elevation_integrate(g.dev.handle, a.handle, None, gp.ctypes.data, 1, C.byref(p), None) == lom.capi.ERR_ARG
    assert L.lom_elevation_integrate(g.dev.handle, a.handle, np.zeros(1, np.int64).ctypes.data, gp.ctypes.data, 1, None, None) == lom.capi.ERR_ARG
    good_lp, good_cp = (1, 2), (1.0, 1.0, 1.0, 1.0)
    for lp in ((0, 1), (1, 0), (1, 5)):
        for call in (lambda: g.dev.layers(lp), lambda: g.dev.cost(lp, good_cp)):
            with pytest.raises(lom.LomError) as e:
                call()
            assert e.value.code == lom.capi.ERR_ARG
    for cp in ((0.0, 1, 1, 1), (1, -1.0, 1, 1), (1, 1, np.nan, 1), (1, 1, 1, np.inf)):
        with pytest.raises(lom.LomError) as e:
            g.dev.cost(good_lp, cp)
        assert e.value.code == lom.capi.ERR_ARG
    for opt, bad in ((lom.capi.ELEV_OPT_TEST_WAVE_MERGE, 2), (77, 0)):
        assert L.lom_elevation_set_option(g.dev.handle, opt, bad) == lom.capi.ERR_ARG
    with pytest.raises(lom.LomError) as e:
        lom.ElevationGrid(0.5, (0, 0), 10, 8193)
    assert e.value.code == lom.capi.ERR_ARG
    assert g.dev.geometry() == dict(resolution=np.float32(0.1), origin_x=-5.0, origin_y=-4.0, width=100, height=80, z_ref=np.float32(-0.4))
    assert L.lom_elevation_device(g.dev.handle) == 0 and L.lom_elevation_stream(g.dev.handle)
    if L.lom_device_count() > 1:                                                        # an archive on another device
        other = lom.ScanArchive(device=1)
        other.addPoints(scans[0])
        with pytest.raises(lom.LomError) as e:
            g.dev.integrate(other, [0], poses[:1], P2)
        assert e.value.code == lom.capi.ERR_ARG
    g.check_cells()
    g.integrate(a, scans, [2, 0], poses[1:3], P2)                                       # the grid and its buffers go on
    g.check_layers(E.layer_params(2, 2))
    # read-back with a cap and with outputs left out
    count = np.zeros(150, np.uint32)
    total = np.full(150, -1, np.int64)
    assert L.lom_elevation_cells(g.dev.handle, count.ctypes.data, None, None, total.ctypes.data, 100) == 8000
    assert np.array_equal(count[:100], g.cells["count"].ravel()[:100]) and not count[100:].any() and (total[100:] == -1).all()
    assert np.array_equal(total[:100], g.cells["sum"].ravel()[:100])
    slope = np.full(8000, 5.0, np.float32)
    lp = lom.elevationLayerParams((2, 2))
    assert L.lom_elevation_layers(g.dev.handle, C.byref(lp), None, None, None, slope.ctypes.data, None, None, 4000) == 0
    assert slope[:4000].tobytes() == E.layers(GEO2, g.cells, E.layer_params(2, 2))["slope"].ravel()[:4000].tobytes() and (slope[4000:] == 5.0).all()


# ---- mirrors ---------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::ElevationGrid of the C++ mirror compiles with plain g++ and leaves what the Python calls leave."""
    exe = cpp_program.build_with_library(tmp_path, "test_elevation.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    n_unknown, n_lethal, n_costed = [int(v) for v in stdout.split()[-3:]]
    # the same grid and points here (tests/cpp/test_elevation.cpp)
    k = np.arange(400)
    pts = np.stack([0.37 * (k % 20) + 0.2, 0.41 * (k // 20) + 0.1, 0.06 * (k % 20) - 0.9 + 0.5 * ((k // 20) == 9)], 1).astype(np.float32)
    poses = np.array([[0.1, 0.1, 0.1, 1, 0, 0, 0], [0.1, 0.3, 0.1, 2, 0, 0, 0.1]])
    ref = E.integrate(GEO1, [pts], [0, 0], poses, E.point_params(-2.0, 1.0, 0.5, 30.0))
    _, summary, _ = E.cost(GEO1, ref["cells"], E.layer_params(1, 2), E.cost_params(0.2, 0.12, 0.2, 0.3))
    assert (n_unknown, n_lethal, n_costed) == (summary["cells_unknown"], summary["cells_lethal"], summary["cells_costed"])
