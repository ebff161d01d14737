"""The occupancy grid on the device against tests/occupancy_ref.py: free, seen, classification, summary and every stats
field exactly equal -- counts are integer sums of bits, there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

from tests import cpp_program
from tests import occupancy_ref as O
from tests import occupancy_scene as OS
from tests.test_vote_gpu import pose_in_room, room_scan

pytestmark = pytest.mark.gpu

WINDOWS = (0, 32, -1)  # no LDS window, the smallest, the default
RULE = O.rule(2, 1, 1)


class Grid:
    """a device grid and the counts the reference expects of it"""

    def __init__(self, lom, geo):
        self.lom, self.geo = lom, geo
        self.dev = lom.OccupancyGrid(geo["resolution"], (geo["origin_x"], geo["origin_y"]), geo["width"], geo["height"])
        self.free = np.zeros((geo["height"], geo["width"]), np.uint32)
        self.seen = np.zeros_like(self.free)

    def window(self, w):
        self.dev.setOption(self.lom.capi.OCC_OPT_TEST_WINDOW, w)

    def slice_max(self, s):
        self.dev.setOption(self.lom.capi.OCC_OPT_TEST_SLICE_MAX, s)

    def check_counts(self):
        free, seen = self.dev.counts()
        assert np.array_equal(free, self.free), np.argwhere(free != self.free)[:10]
        assert np.array_equal(seen, self.seen), np.argwhere(seen != self.seen)[:10]

    def check_classes(self, rule=RULE):
        cls, summary = self.dev.classify(rule)
        want, want_summary = O.classify(self.free, self.seen, rule)
        assert np.array_equal(cls, want) and summary == want_summary
        return want_summary

    def integrate(self, archive, scans, ids, poses, p):
        """device and reference, compared: stats, then the counts"""
        ref = O.integrate(self.geo, scans, ids, poses, p, self.free, self.seen)
        assert not ref["error"]
        st = self.dev.integrate(archive, ids, poses, p)
        assert st == ref["stats"], (st, ref["stats"])
        self.free, self.seen = ref["free"], ref["seen"]
        self.check_counts()
        return ref

    def clear(self):
        self.dev.clear()
        self.free[:], self.seen[:] = 0, 0
        self.check_counts()


def archive_of(lom, scans):
    """(a host cloud with a non-finite coordinate is refused: such a scan goes in from HBM, another handle's staging
    buffers, where it is not looked at)"""
    L, a = lom.capi.lib(), lom.ScanArchive()
    for k, x in enumerate(scans):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
        if np.isfinite(x).all():
            assert a.addPoints(x) == k
            continue
        with pytest.raises(lom.LomError) as e:
            a.addPoints(x)
        assert e.value.code == lom.capi.ERR_ARG and len(a) == k
        ws, dx, dn = lom.VoxelGrid(0.5, 1), C.c_void_p(), C.c_void_p()
        lom.capi.check(L.lom_upload_points(ws.handle, x.ctypes.data, x.ctypes.data, len(x), 12, C.byref(dx), C.byref(dn)), ws.handle)
        lom.capi.check(L.lom_map_status(ws.handle), ws.handle)  # (waits for that handle's copies)
        assert a.addPointsDevice(dx, len(x)) == k
    return a


# ---- 1: hand-written rays --------------------------------------------------------------------------------------------------
GEO1 = O.geometry(0.5, -4.0, -3.0, 45, 37)  # x in [-4, 18.5), y in [-3, 15.5); the width is no multiple of 32
P1 = O.ray_params(z_lo=-1.0, z_hi=0.5, margin=0.25, min_range=1.0, max_range=6.0)
nan, inf = np.nan, np.inf
HAND = [  # (origin, endpoints relative to it): every scan has the identity rotation, so the sensor frame is the map's, moved
    ((2.25, 2.25, 1.0), [  # inside a cell
        [3, 0, 0], [-3, 0, 0], [0, 3, 0], [0, -3, 0],                 # axis-aligned (Dz == 0 as well)
        [2.75, 2.75, 0], [-2.75, 2.75, 0], [-2.25, -2.25, 0.2],       # diagonals
        [3, 1, 0.5], [3, 1, 0.75], [3, 1, -1.0], [3, 1, -1.25],       # just inside and just outside the band, both ends
        [1, 0, 0], [0.75, 0, 0],                                      # L == min_range, L < min_range
        [6, 0, 0], [6.5, 0, 0],                                       # L == max_range, beyond it
        [0, 0, 0], [nan, 0, 0], [inf, 1, 0], [0, -inf, 0], [1, 1, nan], [1, 1, inf],   # zero length, NaN, inf
        [-5.5, -4, 0.1], [2, -5.9, -0.3],                             # leaving the grid
    ]),
    ((2.0, 2.25, 0.0), [[3, 1, 0], [-3, 1, 0], [0, 3, 0], [0, -3, 0], [-2, -2, 0.1]]),   # on a plane x = const
    ((2.0, 2.0, 0.0), [[3, 3, 0], [-3, -3, 0], [3, -3, 0], [-3, 3, 0], [3, 0, 0], [0, -3, 0], [-3, 0, 0], [2, 1, 0.3],
                       [1.5, 1.5, 0], [-2.5, -2.5, 0]]),              # on a corner: exact diagonals through corners
    ((-6.25, 1.3, 0.2), [[5, 0.5, 0], [4, 2, -0.2], [1.5, 0, 0], [-3, 0, 0], [5.9, -0.9, 0.1]]),   # outside, rays enter
    ((30.0, 30.0, 0.0), [[-3, -3, 0], [3, 3, 0]]),                    # far outside: nothing enters
    ((-3.9, -2.9, 0.3), [[4, 0.5, 0], [0.5, 4, 0], [3, 3, -0.5], [-2, -2, 0], [5, 0.1, 0.2]]),   # cell (0, 0): the window
    ((18.4, 15.4, 0.3), [[-4, -0.5, 0], [-0.5, -4, 0], [-3, -3, 0.4], [2, 2, 0], [-5, -0.1, 0.2]]),   # hangs over an edge
]


def test_hand_written_rays(lom):
    scans = [np.asarray(pts, np.float32) for _, pts in HAND]
    poses = np.array([[*o, 1, 0, 0, 0] for o, _ in HAND], np.float64)
    a = archive_of(lom, scans)
    g = Grid(lom, GEO1)
    for w in WINDOWS:
        g.window(w)
        g.clear()
        walked = []
        for k in range(len(HAND)):  # every scan on its own, on top of each other, then all together
            ref = g.integrate(a, scans, [k], poses[k:k + 1], P1)
            walked.append(ref["stats"]["rays_walked"])
        # scan 0: 23 rays; L < min_range, the zero length and the five non-finite ones are not walked
        assert walked == [16, 5, 10, 5, 2, 5, 5]
        ref = g.integrate(a, scans, np.arange(len(HAND)), poses, P1)
        assert ref["stats"]["rays_skipped"] == 7 and ref["stats"]["endpoints_marked"] > 20
        assert ref["free"].max() >= 4 and ref["seen"].max() >= 2
        g.check_classes()
    # what the cases are for, on the reference: the band, the range, the corner tie
    b = O.scan_bits(GEO1, poses[0], scans[0], P1)
    assert b["marked"] == 11 and b["walked"] == 16
    w = O.walk(GEO1, np.float32(HAND[2][0]), np.float32(HAND[2][1]) + np.float32(HAND[2][0]), P1)
    assert w["cell"][w["ray"] == 0][:3].tolist() == [[12, 10], [13, 10], [13, 11]]   # through a corner: x first


# ---- 2: random scans, slices and windows -----------------------------------------------------------------------------------
GEO2 = O.geometry(0.1, -5.0, -4.0, 100, 80)  # the room of tests/test_carve_gpu.py (9 x 7 m) and a margin
P2 = O.ray_params(z_lo=-0.8, z_hi=0.9, margin=0.05, min_range=1.5, max_range=6.0)


@pytest.fixture(scope="module")
def random_scans():
    """65 scans of 200 to 400 points, poses rotated, quaternions not normalised; id 7 is given twice, with two poses"""
    rng = np.random.default_rng(91)
    sizes = rng.integers(200, 401, 65)
    poses = np.stack([pose_in_room(rng, turn=0.6) for _ in range(66)])
    scans = [room_scan(rng, int(n), poses[k])[0] for k, n in enumerate(sizes)]
    ids = np.r_[np.arange(65), 7]
    ref = O.integrate(GEO2, scans, ids, poses, P2)
    assert not ref["error"] and ref["free"].max() > 30 and ref["seen"].max() >= 5 and ref["stats"]["rays_skipped"] > 0
    for k in ("free", "seen"):
        ref[k].setflags(write=False)
    return scans, ids, poses, ref


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("slice_max", [1, 7, 64])
def test_slices_and_windows_give_the_same_bytes(lom, random_scans, slice_max, window):
    scans, ids, poses, ref = random_scans
    a = archive_of(lom, scans)
    g = Grid(lom, GEO2)
    g.slice_max(slice_max)
    g.window(window)
    st = g.dev.integrate(a, ids, poses, P2)
    assert st == ref["stats"]
    g.free, g.seen = ref["free"], ref["seen"]
    g.check_counts()
    g.check_classes(O.rule(3, 2, 1))


def test_options_are_checked(lom):
    L, g = lom.capi.lib(), Grid(lom, GEO1)
    for opt, bad in ((lom.capi.OCC_OPT_TEST_SLICE_MAX, 65), (lom.capi.OCC_OPT_TEST_SLICE_MAX, -1),
                     (lom.capi.OCC_OPT_TEST_WINDOW, 48), (lom.capi.OCC_OPT_TEST_WINDOW, 544), (77, 0)):
        assert L.lom_occupancy_set_option(g.dev.handle, opt, bad) == lom.capi.ERR_ARG
    assert g.dev.geometry() == dict(resolution=0.5, origin_x=-4.0, origin_y=-3.0, width=45, height=37)
    assert L.lom_occupancy_device(g.dev.handle) == 0 and L.lom_occupancy_stream(g.dev.handle)


# ---- 3: calls add up; clear; the bitmaps are at rest -----------------------------------------------------------------------
def test_two_calls_equal_one_and_clear(lom, random_scans):
    scans, ids, poses, _ = random_scans
    a = archive_of(lom, scans[:20])
    one, two = Grid(lom, GEO2), Grid(lom, GEO2)
    ref = one.integrate(a, scans, ids[:20], poses[:20], P2)
    two.integrate(a, scans, ids[:9], poses[:9], P2)
    two.integrate(a, scans, ids[9:20], poses[9:20], P2)
    assert np.array_equal(two.free, ref["free"]) and np.array_equal(two.seen, ref["seen"])
    first = one.dev.counts()
    one.clear()                                             # all zeros
    assert one.check_classes() == dict(cells_free=0, cells_occupied=0, cells_unknown=8000)
    one.integrate(a, scans, ids[:20], poses[:20], P2)       # and the first result again: nothing was left in the bitmaps
    again = one.dev.counts()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    st = one.dev.integrate(a, [], np.empty((0, 7)), P2)     # nothing to do
    assert st == dict(scans=0, rays_walked=0, rays_skipped=0, endpoints_marked=0, cells_visited=0)
    one.check_counts()


# ---- 4: the cloud forms ----------------------------------------------------------------------------------------------------
def test_cloud_forms_equal_the_archive_form(lom, random_scans):
    L = lom.capi.lib()
    scans, ids, poses, _ = random_scans
    x, pose = scans[3], poses[3]
    a = lom.ScanArchive()
    assert a.addPoints(x) == 0
    got_x, got_n = a.get(0)
    assert got_x.tobytes() == x.tobytes() and not got_n.any()            # the points as bytes, zero normals
    want = Grid(lom, GEO2)
    ref = want.integrate(a, [x], [0], pose[None], P2)
    rec = np.zeros(len(x), lom.capi.POINT_XYZIRT)                        # records of 32 bytes that begin with x, y, z
    rec["x"], rec["y"], rec["z"] = x[:, 0], x[:, 1], x[:, 2]
    rec["intensity"] = 7.0
    prm, gp = lom.occupancyRayParams(P2), np.zeros(1, lom.capi.GRAPH_POSE)
    gp["t"][0], gp["q_wxyz"][0] = pose[:3], pose[3:]
    ws, dx, dn = lom.VoxelGrid(0.5, 1), C.c_void_p(), C.c_void_p()        # clouds in HBM: another handle's staging buffers
    for form in ("host12", "host32", "device12", "device32", "archive_device"):
        g = Grid(lom, GEO2)
        st = lom.capi.OccupancyStats()
        if form == "host12":
            assert g.dev.integrateCloud(x, pose, P2) == dict(ref["stats"])
        elif form == "host32":
            rc = L.lom_occupancy_integrate_cloud(g.dev.handle, rec.ctypes.data, len(rec), 32, gp.ctypes.data, C.byref(prm), C.byref(st))
            assert rc == 0 and st.asdict() == ref["stats"]
        else:
            src, stride = (x, 12) if form != "device32" else (rec, 32)
            lom.capi.check(L.lom_upload_points(ws.handle, src.ctypes.data, src.ctypes.data + (0 if stride == 12 else 12),
                                               len(src), stride, C.byref(dx), C.byref(dn)), ws.handle)
            lom.capi.check(L.lom_map_status(ws.handle), ws.handle)         # (waits for that handle's copies)
            if form == "archive_device":
                a2 = lom.ScanArchive()
                assert a2.addPointsDevice(dx, len(src)) == 0
                assert a2.get(0)[0].tobytes() == x.tobytes() and not a2.get(0)[1].any()
                assert g.dev.integrate(a2, [0], pose[None], P2) == ref["stats"]
            else:
                assert g.dev.integrateCloud(None, pose, P2, device_ptr=dx, n=len(src), stride_bytes=stride) == ref["stats"]
        g.free, g.seen = ref["free"], ref["seen"]
        g.check_counts()
    g = Grid(lom, GEO2)                                                   # n == 0: LOM_OK, nothing changes
    assert g.dev.integrateCloud(np.zeros((0, 3), np.float32), pose, P2)["rays_walked"] == 0
    g.check_counts()
    # classify_device: the same bytes, left in HBM (read back through a map handle's copy would need one; compare sizes
    # and the summary through the host form instead)
    d_out = C.c_void_p()
    r = lom.occupancyRule(RULE)
    assert L.lom_occupancy_classify_device(want.dev.handle, C.byref(r), C.byref(d_out)) == 0 and d_out.value
    want.check_classes()


# ---- 5: the corridor scene -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mover", [True, False])
def test_corridor_scene_equals_the_reference(lom, mover):
    """Only equality is asserted here; the scene's conditions are the reference's (tests/test_occupancy_host.py)."""
    from tests import vote_scene as S
    s, ref = S.scene(mover), OS.reference(mover)
    a = archive_of(lom, [x for x, _ in s["scans"]])
    g = Grid(lom, OS.GEO)
    assert g.dev.integrate(a, s["ids"], s["poses"], OS.PARAMS) == ref["stats"]
    g.free, g.seen = ref["free"], ref["seen"]
    g.check_counts()
    cls, summary = g.dev.classify(OS.RULE)
    assert np.array_equal(cls, ref["cls"]) and summary == ref["summary"]


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_counts_unchanged(lom, random_scans):
    L = lom.capi.lib()
    scans, ids, poses, _ = random_scans
    a = archive_of(lom, scans[:3])
    g = Grid(lom, GEO2)
    g.integrate(a, scans, [0, 1, 2], poses[:3], P2)
    zero = lom.capi.OccupancyStats().asdict()

    def refused(code, ids_, poses_, prm=P2):
        ids64, gp = np.ascontiguousarray(ids_, np.int64), np.zeros(len(ids_), lom.capi.GRAPH_POSE)
        pp = np.asarray(poses_, np.float64).reshape(-1, 7)
        gp["t"], gp["q_wxyz"] = pp[:, :3], pp[:, 3:]
        st, p = lom.capi.OccupancyStats(), lom.occupancyRayParams(prm)
        st.scans = 9
        assert L.lom_occupancy_integrate(g.dev.handle, a.handle, ids64.ctypes.data, gp.ctypes.data, len(ids64), C.byref(p),
                                         C.byref(st)) == code, (ids_, prm)
        assert st.asdict() == zero and L.lom_occupancy_last_error(g.dev.handle)
        x = np.ascontiguousarray(scans[0])
        if len(ids64) == 1 and ids64[0] == 0:  # the cloud form refuses the same pose and parameters
            assert L.lom_occupancy_integrate_cloud(g.dev.handle, x.ctypes.data, len(x), 12, gp.ctypes.data, C.byref(p), C.byref(st)) == code
        g.check_counts()

    for change in (dict(z_lo=0.0), dict(z_lo=0.2), dict(z_hi=0.0), dict(z_hi=np.inf), dict(margin=-0.1), dict(margin=np.nan),
                   dict(min_range=0.0), dict(max_range=0.2), dict(max_range=np.inf), dict(max_range=0.1 * 2.0 ** 20 * 1.01)):
        refused(lom.capi.ERR_ARG, [0], poses[:1], dict(P2, **change))
    for ids_, p in (([3], poses[:1]), ([-1], poses[:1]), ([0], [[0, 0, 0, 0, 0, 0, 0.0]]), ([0, 1], [poses[0], [np.nan, 0, 0, 1, 0, 0, 0]])):
        refused(lom.capi.ERR_ARG, ids_, p)
    refused(lom.capi.ERR_RANGE, [0], [[0.1 * 2.0 ** 30 * 1.01, 0, 0, 1, 0, 0, 0]])     # an origin cell beyond 2^30
    refused(lom.capi.ERR_RANGE, [1, 0], [poses[1], [0, -1e300, 0, 1, 0, 0, 0]])         # rounds to -inf in f32
    assert O.integrate(GEO2, scans, [1, 0], [poses[1], [0, -1e300, 0, 1, 0, 0, 0]], P2)["error"]
    g.dev.integrate(a, [0], [[0.1 * 2.0 ** 30 * 0.9, 0, 0, 1, 0, 0, 0]], P2)            # inside the range, far from the grid: legal
    g.check_counts()
    x = np.ascontiguousarray(scans[0])
    gp, p = np.zeros(1, lom.capi.GRAPH_POSE), lom.occupancyRayParams(P2)
    gp["q_wxyz"][0, 0] = 1.0
    for stride in (8, 14):
        assert L.lom_occupancy_integrate_cloud(g.dev.handle, x.ctypes.data, len(x), stride, gp.ctypes.data, C.byref(p), None) == lom.capi.ERR_ARG
    assert L.lom_occupancy_integrate_cloud(g.dev.handle, None, len(x), 12, gp.ctypes.data, C.byref(p), None) == lom.capi.ERR_ARG
    assert L.lom_occupancy_integrate_cloud(g.dev.handle, x.ctypes.data, len(x), 12, None, C.byref(p), None) == lom.capi.ERR_ARG
    assert L.lom_occupancy_integrate(g.dev.handle, a.handle, None, gp.ctypes.data, 1, C.byref(p), None) == lom.capi.ERR_ARG
    assert L.lom_occupancy_integrate(g.dev.handle, a.handle, np.zeros(1, np.int64).ctypes.data, gp.ctypes.data, 1, None, None) == lom.capi.ERR_ARG
    for bad_rule in ((0, 1, 1), (1, 1, 0)):
        with pytest.raises(lom.LomError) as e:
            g.dev.classify(bad_rule)
        assert e.value.code == lom.capi.ERR_ARG
    with pytest.raises(lom.LomError) as e:
        lom.OccupancyGrid(0.0, (0, 0), 10, 10)
    assert e.value.code == lom.capi.ERR_ARG
    if L.lom_device_count() > 1:                                                        # an archive on another device
        other = lom.ScanArchive(device=1)
        other.addPoints(scans[0])
        with pytest.raises(lom.LomError) as e:
            g.dev.integrate(other, [0], poses[:1], P2)
        assert e.value.code == lom.capi.ERR_ARG
    g.check_counts()
    g.integrate(a, scans, [2, 0], poses[1:3], P2)                                       # the grid and its buffers go on
    g.check_classes()


# ---- mirrors ---------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::OccupancyGrid and ScanArchive::addPoints of the C++ mirror compile with plain g++ and leave what the Python
    calls leave."""
    exe = cpp_program.build_with_library(tmp_path, "test_occupancy.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    n_free, n_occ = [int(v) for v in stdout.split()[-2:]]
    # the same grid and scans here (tests/cpp/test_occupancy.cpp)
    pts = np.array([[6.1, 0.3 * k - 2.0, 0.05 * k - 0.3] for k in range(12)], np.float32)
    poses = np.array([[0.1, 0.1, 0.1, 1, 0, 0, 0], [0.1, 0.3, 0.1, 2, 0, 0, 0.1]])
    ref = O.integrate(GEO1, [pts], [0, 0], poses, O.ray_params(-1.0, 1.0, 0.0, 0.5, 12.0))
    _, summary = O.classify(ref["free"], ref["seen"], O.rule(1, 1, 1))
    assert (n_free, n_occ) == (summary["cells_free"], summary["cells_occupied"])
