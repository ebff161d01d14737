"""lom_odometry_archive_scan and lom_odometry_rebuild_keyframe on a short synthetic drive (the generator of
tests/test_pipeline.py).  Every stored scan is compared byte for byte with the one an odometry with host stages
(LOM_HOST_FRONTEND=1) stores from the same frames, and the last one with the update cloud restated from getTempCloud().
Then the poses are nudged as a pose graph would, odometry A rebuilds its keyframe from the archive, odometry B is put into the
same state by debugSetState with a keyframe built from tests/assemble_ref.py and the library's insert, and both go on:
keyframes, poses and frame stats are compared as bytes.  No tolerance anywhere."""
import numpy as np
import pytest

from lidar_odometry_demo_amd import synth
from tests import assemble_ref as ref

pytestmark = pytest.mark.gpu

N_FRAMES = 12
N_AZ = 600


def _frame(k):
    return synth.make_sequence_frame(k, n_az=N_AZ)


def _pose_bits(p):
    return np.asarray(p.translation, np.float32).tobytes() + np.asarray(p.rotation, np.float32).tobytes()


def _drive(lom, archive=None):
    o = lom.LidarOdometry()
    poses, ids = [], []
    for k in range(N_FRAMES):
        o.processCloud(_frame(k))
        poses.append(o.getCurrentPose())
        if archive is not None:
            ids.append(o.archiveScan(archive))
    return o, poses, ids


@pytest.fixture(scope="module")
def drives(lom):
    import os

    arch, arch_host = lom.ScanArchive(1, 1), lom.ScanArchive()
    with pytest.raises(lom.LomError) as e:
        lom.LidarOdometry().archiveScan(arch)
    assert e.value.code == lom.capi.ERR_STATE and len(arch) == 0
    a, poses_a, ids = _drive(lom, arch)
    b, poses_b, _ = _drive(lom)
    os.environ["LOM_HOST_FRONTEND"] = "1"
    try:
        h, poses_h, ids_h = _drive(lom, arch_host)
    finally:
        del os.environ["LOM_HOST_FRONTEND"]
    return dict(a=a, b=b, h=h, arch=arch, arch_host=arch_host, poses_a=poses_a, poses_b=poses_b, poses_h=poses_h, ids=ids,
                ids_h=ids_h)


def test_archive_scan_stores_the_update_cloud_and_moves_nothing(lom, drives):
    d = drives
    assert d["ids"] == list(range(N_FRAMES)) == d["ids_h"] and d["h"].stats["host_stages"] == 1 and d["a"].stats["host_stages"] == 0
    # archiving reads only: the drive's poses are those of a drive that never touched an archive
    assert [_pose_bits(p) for p in d["poses_a"]] == [_pose_bits(p) for p in d["poses_b"]]
    assert d["a"].getFullKeyFrameCloud().tobytes() == d["b"].getFullKeyFrameCloud().tobytes()
    assert d["a"].stats == d["b"].stats
    # device stages and host stages store the same bytes, frame by frame (their poses agree, so their frames do)
    assert [_pose_bits(p) for p in d["poses_a"]] == [_pose_bits(p) for p in d["poses_h"]]
    for k in range(N_FRAMES):
        (x, n), (hx, hn) = d["arch"].get(k), d["arch_host"].get(k)
        assert len(x) > 100 and x.tobytes() == hx.tobytes() and n.tobytes() == hn.tobytes()
    assert d["arch"].scanSize(N_FRAMES - 1) == d["a"].stats["update_points"]
    # the last one against the update cloud restated from the deskewed cloud: classify, range filter, down-sampling
    o = d["a"]
    pxyz, pnrm, _, _ = lom.classify(o.getTempCloud())
    fx, fn = lom.rangeFilter(pxyz, pnrm, o.params.lidar_min_range, o.params.lidar_max_range)
    dx, dn = lom.VoxelGrid(0.5, 1).downsample(fx, fn, o.params.keyframe_update_voxel_size)
    x, n = d["arch"].get(N_FRAMES - 1)
    assert x.tobytes() == dx.tobytes() and n.tobytes() == dn.tobytes()


def test_rebuild_keyframe_and_go_on(lom, drives):
    d = drives
    a, b, arch = d["a"], d["b"], d["arch"]
    # the keyframe poses as f64, nudged as an optimisation would: small, distinct corrections
    poses = np.array([np.concatenate([p.translation.astype(np.float64), p.rotation.astype(np.float64)]) for p in d["poses_a"]])
    for k in range(N_FRAMES):
        poses[k, :3] += 1e-3 * (k + 1) * np.array([1.0, -0.5, 0.25])
        poses[k, 3:] += 1e-4 * (k + 1) * np.array([0.0, 1.0, -1.0, 0.5])  # (normalised on entry)
    ids = np.arange(N_FRAMES)[::-1]  # newest first
    order = poses[::-1]
    last = poses[-1]
    new_current = lom.Pose3D(last[:3].astype(np.float32), (last[3:] / np.linalg.norm(last[3:])).astype(np.float32))
    # refusals leave everything as it was
    with pytest.raises(lom.LomError) as e:
        lom.LidarOdometry().rebuildKeyframe(arch, ids, order, new_current)
    assert e.value.code == lom.capi.ERR_STATE
    # B: the same state through the existing hook, its keyframe from the reference cloud and the library's insert
    scans = [arch.get(k) for k in range(N_FRAMES)]
    prm = b.params
    cx, cn = ref.concatenated(scans, ids, order, centre=new_current.translation, radius=prm.keyframe_cleanup_range)
    want = lom.VoxelGrid(prm.keyframe_voxel_size, prm.keyframe_max_points_cnt)
    want.addCloud(cx, cn)
    kx, kn = want.getCloud()
    current, previous = d["poses_b"][-1], d["poses_b"][-2]
    corr = new_current.compose(current.inverse())
    b.debugSetState(corr.compose(previous), new_current, kx, kn)
    # A: the call under test
    st = a.rebuildKeyframe(arch, ids, order, new_current)
    assert st == dict(scans=N_FRAMES, points_in=arch.pointCount(), points_kept=len(cx), voxels_before=0,
                      voxels_after=want.size(), points_stored_after=want.pointCount())
    assert 0 < st["points_kept"] and st["voxels_after"] > 100
    assert _pose_bits(a.getCurrentPose()) == _pose_bits(new_current) == _pose_bits(b.getCurrentPose())
    ax, an = a.getFullKeyFrameCloudWithNormals()
    bx, bn = b.getFullKeyFrameCloudWithNormals()
    assert ax.tobytes() == bx.tobytes() == kx.tobytes() and an.tobytes() == bn.tobytes() == kn.tobytes()
    for k in (N_FRAMES, N_FRAMES + 1):
        a.processCloud(_frame(k))
        b.processCloud(_frame(k))
        assert _pose_bits(a.getCurrentPose()) == _pose_bits(b.getCurrentPose())
        sa, sb = a.stats, b.stats
        assert sa == sb and sa["initialised_keyframe"] == 0 and sa["outer_iterations"] > 0
    ax, an = a.getFullKeyFrameCloudWithNormals()
    bx, bn = b.getFullKeyFrameCloudWithNormals()
    assert ax.tobytes() == bx.tobytes() and an.tobytes() == bn.tobytes()
    # a failing assembly: the old poses stay, the keyframe is reported cleared and the next frame initialises it anew
    before = _pose_bits(a.getCurrentPose())
    with pytest.raises(lom.LomError) as e:
        a.rebuildKeyframe(arch, [N_FRAMES + 5], order[:1], new_current)
    assert e.value.code == lom.capi.ERR_ARG and _pose_bits(a.getCurrentPose()) == before
    assert len(a.getFullKeyFrameCloud()) == 0
    a.processCloud(_frame(N_FRAMES + 2))
    assert a.stats["initialised_keyframe"] == 1 and a.stats["keyframe_voxels"] > 0
