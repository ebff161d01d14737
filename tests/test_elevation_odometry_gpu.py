"""lom_odometry_elevation_scan on a short synthetic drive (the generator of tests/test_pipeline.py), once with device stages
and once with LOM_HOST_FRONTEND=1: the grid the odometry fills frame by frame equals the grid of
integrateCloud(getTempCloud) at getCurrentPose, and the grid integrated afterwards from the archived deskewed clouds at
the same poses in one call; the drive's poses, keyframe and stats are those of a drive that never made the calls.  The
cells are compared exactly."""
import os

import numpy as np
import pytest

from lidar_odometry_demo_amd import synth
from tests import elevation_ref as E

pytestmark = pytest.mark.gpu

N_FRAMES = 4
N_AZ = 600
GEO = E.geometry(0.25, -40.0, -15.0, 400, 120, 0.0)
PARAMS = E.point_params(z_lo=-3.0, z_hi=1.0, min_range=2.0, max_range=40.0)


def _grid(lom):
    return lom.ElevationGrid(GEO["resolution"], (GEO["origin_x"], GEO["origin_y"]), GEO["width"], GEO["height"], GEO["z_ref"])


def _pose7(p):
    """the f32 pose widened, as lom_graph_pose_from_f32 does"""
    return np.concatenate([np.asarray(p.translation, np.float32), np.asarray(p.rotation, np.float32)]).astype(np.float64)


def _pose_bits(p):
    return np.asarray(p.translation, np.float32).tobytes() + np.asarray(p.rotation, np.float32).tobytes()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.cells(), b.cells()))


def _drive(lom, with_calls):
    o = lom.LidarOdometry()
    by_odometry, by_cloud, archive = _grid(lom), _grid(lom), lom.ScanArchive()
    if with_calls:
        with pytest.raises(lom.LomError) as e:
            o.elevationScan(by_odometry, PARAMS)
        assert e.value.code == lom.capi.ERR_STATE                       # before the first frame
        assert not by_odometry.cells()[0].any()
    bits, poses, stats = [], [], []
    for k in range(N_FRAMES):
        o.processCloud(synth.make_sequence_frame(k, n_az=N_AZ))
        pose = o.getCurrentPose()
        bits.append(_pose_bits(pose))
        if not with_calls:
            continue
        st = o.elevationScan(by_odometry, PARAMS)
        cloud = o.getTempCloud()
        xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
        assert by_cloud.integrateCloud(xyz, _pose7(pose), PARAMS) == st
        assert st["scans"] == 1 and st["points"] == len(cloud) and st["points_marked"] > 1000 and st["points_out_of_height"] == 0
        assert o.archiveDeskewed(archive) == k
        poses.append(_pose7(pose))
        stats.append(st)
    return dict(o=o, bits=bits, by_odometry=by_odometry, by_cloud=by_cloud, archive=archive, poses=poses, stats=stats)


@pytest.mark.parametrize("host_frontend", [False, True])
def test_elevation_scan(lom, host_frontend):
    if host_frontend:
        os.environ["LOM_HOST_FRONTEND"] = "1"
    try:
        d = _drive(lom, True)
        plain = _drive(lom, False)
    finally:
        os.environ.pop("LOM_HOST_FRONTEND", None)
    assert d["o"].stats["host_stages"] == (1 if host_frontend else 0)
    count, zmin, zmax, total = d["by_odometry"].cells()
    assert count.sum() == sum(s["points_marked"] for s in d["stats"]) and (count > 0).sum() > 2000
    assert (zmin[count > 0] <= zmax[count > 0]).all() and (zmin[count == 0] == E.I32_MAX).all()
    assert _same(d["by_odometry"], d["by_cloud"])
    # the archived deskewed clouds at the same poses, in one call
    from_archive = _grid(lom)
    st = from_archive.integrate(d["archive"], np.arange(N_FRAMES), np.stack(d["poses"]), PARAMS)
    assert _same(d["by_odometry"], from_archive)
    for key in ("points", "points_marked", "points_out_of_height", "cells_new"):
        assert st[key] == sum(s[key] for s in d["stats"])
    # the layers of the two are the same bytes as well
    lp = E.layer_params(2, 2)
    a, b = d["by_odometry"].layers(lp), from_archive.layers(lp)
    assert all(a[k].tobytes() == b[k].tobytes() for k in E.LAYERS) and np.isfinite(a["slope"]).sum() > 1000
    # reads only: the poses and the keyframe of a drive that never made the calls
    assert d["bits"] == plain["bits"]
    assert d["o"].getFullKeyFrameCloud().tobytes() == plain["o"].getFullKeyFrameCloud().tobytes()
    assert d["o"].stats == plain["o"].stats
