"""lom_odometry_occupancy_scan and lom_odometry_archive_deskewed on a short synthetic drive (the generator of
tests/test_pipeline.py), once with device stages and once with LOM_HOST_FRONTEND=1: the grid the odometry fills frame by
frame equals the grid of integrate_cloud(getTempCloud) at getCurrentPose, and the grid integrated afterwards from the
archived deskewed clouds at the same poses; the drive's poses are those of a drive that never made the calls.  Counts are
compared exactly."""
import os

import numpy as np
import pytest

from lidar_odometry_demo_amd import synth
from tests import occupancy_ref as O

pytestmark = pytest.mark.gpu

N_FRAMES = 4
N_AZ = 600
GEO = O.geometry(0.25, -40.0, -15.0, 400, 120)
PARAMS = O.ray_params(z_lo=-1.5, z_hi=0.6, margin=0.1, min_range=2.0, max_range=40.0)


def _grid(lom):
    return lom.OccupancyGrid(GEO["resolution"], (GEO["origin_x"], GEO["origin_y"]), GEO["width"], GEO["height"])


def _pose7(p):
    """the f32 pose widened, as lom_graph_pose_from_f32 does"""
    return np.concatenate([np.asarray(p.translation, np.float32), np.asarray(p.rotation, np.float32)]).astype(np.float64)


def _pose_bits(p):
    return np.asarray(p.translation, np.float32).tobytes() + np.asarray(p.rotation, np.float32).tobytes()


def _same(a, b):
    (fa, sa), (fb, sb) = a.counts(), b.counts()
    return np.array_equal(fa, fb) and np.array_equal(sa, sb)


def _drive(lom, with_calls):
    o = lom.LidarOdometry()
    by_odometry, by_cloud, archive = _grid(lom), _grid(lom), lom.ScanArchive()
    if with_calls:
        for call in (lambda: o.occupancyScan(by_odometry, PARAMS), lambda: o.archiveDeskewed(archive)):
            with pytest.raises(lom.LomError) as e:
                call()
            assert e.value.code == lom.capi.ERR_STATE                   # before the first frame
        assert len(archive) == 0 and not by_odometry.counts()[0].any()
    bits, poses, stats = [], [], []
    for k in range(N_FRAMES):
        o.processCloud(synth.make_sequence_frame(k, n_az=N_AZ))
        pose = o.getCurrentPose()
        bits.append(_pose_bits(pose))
        if not with_calls:
            continue
        st = o.occupancyScan(by_odometry, PARAMS)
        cloud = o.getTempCloud()
        xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
        assert by_cloud.integrateCloud(xyz, _pose7(pose), PARAMS) == st
        assert st["scans"] == 1 and st["rays_walked"] + st["rays_skipped"] == len(cloud) and st["rays_walked"] > 1000
        assert o.archiveDeskewed(archive) == k
        got, nrm = archive.get(k)
        assert got.tobytes() == np.ascontiguousarray(xyz, np.float32).tobytes() and not nrm.any()
        poses.append(_pose7(pose))
        stats.append(st)
    return dict(o=o, bits=bits, by_odometry=by_odometry, by_cloud=by_cloud, archive=archive, poses=poses, stats=stats)


@pytest.mark.parametrize("host_frontend", [False, True])
def test_occupancy_scan_and_archive_deskewed(lom, host_frontend):
    if host_frontend:
        os.environ["LOM_HOST_FRONTEND"] = "1"
    try:
        d = _drive(lom, True)
        plain = _drive(lom, False)
    finally:
        os.environ.pop("LOM_HOST_FRONTEND", None)
    assert d["o"].stats["host_stages"] == (1 if host_frontend else 0)
    free, seen = d["by_odometry"].counts()
    assert free.max() == N_FRAMES and seen.max() >= 2 and (free > 0).sum() > 5000
    assert _same(d["by_odometry"], d["by_cloud"])
    # the archived deskewed clouds at the same poses, in one call
    from_archive = _grid(lom)
    st = from_archive.integrate(d["archive"], np.arange(N_FRAMES), np.stack(d["poses"]), PARAMS)
    assert _same(d["by_odometry"], from_archive)
    for key in ("rays_walked", "rays_skipped", "endpoints_marked", "cells_visited"):
        assert st[key] == sum(s[key] for s in d["stats"])
    # reads only: the poses and the keyframe of a drive that never made the calls
    assert d["bits"] == plain["bits"]
    assert d["o"].getFullKeyFrameCloud().tobytes() == plain["o"].getFullKeyFrameCloud().tobytes()
    assert d["o"].stats == plain["o"].stats
