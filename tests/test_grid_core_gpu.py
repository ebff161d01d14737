"""What the occupancy and the elevation grid share on the host (csrc/grid_handle.hpp), on the device: one ScanArchive, one
OccupancyGrid and one ElevationGrid in interleaved calls -- archive and cloud forms, the packed upload of a strided host
cloud, an archive cleared and filled again between two integrates -- with counts, cells and stats exactly those of
tests/occupancy_ref.py and tests/elevation_ref.py; and refusals, which leave both grids as they were and name their reason
in last_error.  Every stream here is the handle's own: what is compared is also the ordering between them."""
import ctypes as C

import numpy as np
import pytest

from tests import elevation_ref as E
from tests import occupancy_ref as O

pytestmark = pytest.mark.gpu

OGEO = O.geometry(0.5, -4.0, -4.0, 16, 16)  # 16 x 16 cells of 0.5 m
EGEO = E.geometry(0.5, -4.0, -4.0, 16, 16, 0.25)
RAY = O.ray_params(z_lo=-1.0, z_hi=1.0, margin=0.25, min_range=0.5, max_range=6.0)
PNT = E.point_params(z_lo=-1.0, z_hi=1.0, min_range=0.5, max_range=6.0)
POSES = np.array([[0.3, -0.2, 0.1, 1, 0, 0, 0], [-1.1, 0.9, 0.0, 0.9, 0, 0, 0.3], [1.4, 1.2, -0.1, 0.7, 0.02, -0.03, -0.6]], np.float64)


def three_scans():
    """three scans of about 200 points in the sensor frame, some of them beyond the grid and the ranges"""
    rng = np.random.default_rng(20251)
    return [np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-1.2, 1.2, n)]).astype(np.float32)
            for n in (199, 200, 203)]


class Pair:
    """the two device grids and what the references expect of them"""

    def __init__(self, lom):
        self.lom, self.L = lom, lom.capi.lib()
        self.occ = lom.OccupancyGrid(0.5, (-4.0, -4.0), 16, 16)
        self.elev = lom.ElevationGrid(0.5, (-4.0, -4.0), 16, 16, 0.25)
        self.free, self.seen = np.zeros((16, 16), np.uint32), np.zeros((16, 16), np.uint32)
        self.cells = E.empty_cells(EGEO)

    def expect_occ(self, scans, ids, poses, st):
        ref = O.integrate(OGEO, scans, ids, poses, RAY, self.free, self.seen)
        assert not ref["error"] and st == ref["stats"], (st, ref["stats"])
        self.free, self.seen = ref["free"], ref["seen"]
        self.check()

    def expect_elev(self, scans, ids, poses, st):
        ref = E.integrate(EGEO, scans, ids, poses, PNT, self.cells)
        assert not ref["error"] and st == ref["stats"], (st, ref["stats"])
        self.cells = ref["cells"]
        self.check()

    def check(self):
        free, seen = self.occ.counts()
        assert np.array_equal(free, self.free) and np.array_equal(seen, self.seen)
        for k, got in zip(("count", "zmin", "zmax", "sum"), self.elev.cells()):
            assert np.array_equal(got, self.cells[k]), k

    def occ_cloud_strided(self, xyz, stride_floats, pose_ptr):
        """lom_occupancy_integrate_cloud on records of stride_floats floats: (rc, stats)"""
        rec = np.full((len(xyz), stride_floats), 7.0, np.float32)
        rec[:, :3] = xyz
        st, p = self.lom.capi.OccupancyStats(), self.lom.occupancyRayParams(RAY)
        rc = self.L.lom_occupancy_integrate_cloud(self.occ.handle, rec.ctypes.data, len(rec), 4 * stride_floats, pose_ptr,
                                                  C.byref(p), C.byref(st))
        return rc, st.asdict()


def pose_of(lom, k):
    return lom._graph_poses(POSES[k:k + 1])


def test_interleaved_calls_on_one_archive(lom):
    scans, g, a = three_scans(), Pair(lom), lom.ScanArchive()
    assert a.addPoints(scans[0]) == 0 and a.addPoints(scans[1]) == 1
    g.expect_occ(scans, [0, 1], POSES[:2], g.occ.integrate(a, [0, 1], POSES[:2], RAY))
    g.expect_elev(scans, [1, 0], POSES[:2], g.elev.integrate(a, [1, 0], POSES[:2], PNT))
    assert a.addPoints(scans[2]) == 2
    g.expect_elev(scans, [2], POSES[2:], g.elev.integrateCloud(scans[2], POSES[2], PNT))
    pose = pose_of(lom, 2)
    rc, st = g.occ_cloud_strided(scans[2], 5, pose.ctypes.data)  # 20-byte records: the packed upload
    assert rc == 0
    g.expect_occ(scans, [2], POSES[2:], st)
    # the archive again, with other clouds behind the same ids: what the grids read next is what was added last
    a.clear()
    again = [scans[2], scans[0], scans[1]]
    assert [a.addPoints(x) for x in again] == [0, 1, 2]
    g.expect_occ(again, [0, 1, 2], POSES, g.occ.integrate(a, [0, 1, 2], POSES, RAY))
    g.expect_elev(again, [2, 2, 0], POSES, g.elev.integrate(a, [2, 2, 0], POSES, PNT))


def refused(lom, grid, call, text):
    """`call` raises LomError(LOM_ERR_ARG) or returns LOM_ERR_ARG; the grid's last error is `text`, which names the family"""
    try:
        rc = call()
    except lom.LomError as e:
        rc = e.code
        assert str(e).endswith(": " + text)
    assert rc == lom.capi.ERR_ARG
    last = getattr(lom.capi.lib(), "lom_" + text.split(":")[0] + "_last_error")(grid.handle)
    assert last.decode() == text


def filled_pair(lom):
    scans, g, a = three_scans(), Pair(lom), lom.ScanArchive()
    assert a.addPoints(scans[0]) == 0
    g.expect_occ(scans, [0], POSES[:1], g.occ.integrate(a, [0], POSES[:1], RAY))
    g.expect_elev(scans, [0], POSES[:1], g.elev.integrate(a, [0], POSES[:1], PNT))
    assert g.seen.any() and g.cells["count"].any()
    return scans, g, a


def test_a_refusal_leaves_both_grids_unchanged(lom):
    scans, g, a = filled_pair(lom)
    L, x, pose = g.L, np.ascontiguousarray(scans[1]), pose_of(lom, 1)
    est, ep = lom.capi.ElevationStats(), lom.elevationPointParams(PNT)
    cloud = "{}: a cloud, a pose and a stride >= 12 that is a multiple of 4"
    # a NULL pose
    refused(lom, g.occ, lambda: g.occ_cloud_strided(x, 3, None)[0], cloud.format("occupancy"))
    refused(lom, g.elev, lambda: L.lom_elevation_integrate_cloud(g.elev.handle, x.ctypes.data, len(x), 12, None, C.byref(ep),
                                                                C.byref(est)), cloud.format("elevation"))
    g.check()
    # a stride that is no multiple of 4, and one below 12
    for stride in (14, 8):
        st, p = lom.capi.OccupancyStats(), lom.occupancyRayParams(RAY)
        refused(lom, g.occ, lambda: L.lom_occupancy_integrate_cloud(g.occ.handle, x.ctypes.data, len(x), stride, pose.ctypes.data,
                                                                   C.byref(p), C.byref(st)), cloud.format("occupancy"))
        refused(lom, g.elev, lambda: L.lom_elevation_integrate_cloud(g.elev.handle, x.ctypes.data, len(x), stride, pose.ctypes.data,
                                                                    C.byref(ep), C.byref(est)), cloud.format("elevation"))
    g.check()
    # an id that is not in the archive, behind one that is
    refused(lom, g.occ, lambda: g.occ.integrate(a, [0, 1], POSES[:2], RAY), "occupancy: scan 1 of the call: no scan with this id")
    refused(lom, g.elev, lambda: g.elev.integrate(a, [0, 1], POSES[:2], PNT), "elevation: scan 1 of the call: no scan with this id")
    g.check()
    # and the grids still take a call
    g.expect_occ(scans, [0], POSES[1:2], g.occ.integrate(a, [0], POSES[1:2], RAY))
    g.expect_elev(scans, [0], POSES[1:2], g.elev.integrate(a, [0], POSES[1:2], PNT))


def test_a_grid_and_an_archive_on_different_devices(lom):
    if lom.capi.lib().lom_device_count() < 2:
        pytest.skip("needs a second device")
    scans, g, _ = filled_pair(lom)
    far = lom.ScanArchive(device=1)
    assert far.addPoints(scans[1]) == 0
    where = "{}: the grid and the archive live on different devices"
    refused(lom, g.occ, lambda: g.occ.integrate(far, [0], POSES[:1], RAY), where.format("occupancy"))
    refused(lom, g.elev, lambda: g.elev.integrate(far, [0], POSES[:1], PNT), where.format("elevation"))
    g.check()
