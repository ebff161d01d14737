"""Scan votes in lom_odometry_rebuild_keyframe (lom_odometry_set_rebuild_votes) on the 12-frame mover sequence of
tests/test_carve_odometry_gpu.py: every frame is archived, then the keyframe is rebuilt at the odometry's own poses.
With votes unset the rebuild is byte for byte what it was; with votes set the keyframe equals lom_map_assemble followed by
lom_map_carve_scans on a second map, and the odometry goes on aligning.  The ghost points that the rebuild brings back
in the mover's swept box, with and without votes, are recorded in profiles/vote_odometry.json -- recorded, not asserted:
the update clouds exist only on the device, so no reference of this project can say what they should be."""
import json
import os

import numpy as np
import pytest

from tests import vote_ref as V
from tests.conftest import ROOT
from tests.test_carve_odometry_gpu import N_FRAMES, SWEPT, _frame

pytestmark = pytest.mark.gpu

VOTES = V.params(margin=0.4, min_range=4.0, max_range=60.0, clearance=0.75, min_free_scans=3, free_per_seen=2)
SWEPT_ALL = np.r_[SWEPT[:4], 15.0, SWEPT[5]]  # the box the mover sweeps over all 12 frames


def _pose64(p):
    return np.concatenate([p.translation.astype(np.float64), p.rotation.astype(np.float64)])


def _drive(lom, how):
    """12 frames with the mover, each archived; then the rebuild at the drive's own poses"""
    o, arch = lom.LidarOdometry(), lom.ScanArchive()
    if how == "set":
        o.setRebuildVotes(VOTES)
    elif how == "touched":
        o.setRebuildVotes(VOTES)
        o.setRebuildVotes(None)
    poses = []
    for k in range(N_FRAMES):
        o.processCloud(_frame(k, True))
        poses.append(_pose64(o.getCurrentPose()))
        assert o.archiveScan(arch) == k
    poses = np.stack(poses)
    ids = np.arange(N_FRAMES)[::-1]  # newest first
    st = o.rebuildKeyframe(arch, ids, poses[::-1], o.getCurrentPose())
    return dict(o=o, arch=arch, ids=ids, poses=poses[::-1].copy(), stats=st, full=o.getFullKeyFrameCloudWithNormals())


def _ghosts(xyz):
    return int(np.all((xyz >= SWEPT_ALL[:3]) & (xyz <= SWEPT_ALL[3:]), axis=1).sum())


@pytest.fixture(scope="module")
def drives(lom):
    return {how: _drive(lom, how) for how in ("never", "touched", "set")}


def test_votes_unset_change_nothing(drives):
    never, touched = drives["never"], drives["touched"]
    assert never["full"][0].tobytes() == touched["full"][0].tobytes() and never["full"][1].tobytes() == touched["full"][1].tobytes()
    assert never["stats"] == touched["stats"] and len(never["full"][0]) > 1000
    assert never["o"].rebuildVoteStats() is None and touched["o"].rebuildVoteStats() is None


def test_votes_set_equal_assemble_and_carve_scans_and_the_odometry_goes_on(lom, drives):
    d = drives["set"]
    o = d["o"]
    prm = o.params
    want = lom.VoxelGrid(prm.keyframe_voxel_size, prm.keyframe_max_points_cnt)
    ast = want.assemble(d["arch"], d["ids"], d["poses"], centre=o.getCurrentPose().translation, radius=prm.keyframe_cleanup_range)
    vst = want.carveScans(d["arch"], d["ids"], d["poses"], VOTES)
    wx, wn = want.getCloud()
    assert d["full"][0].tobytes() == wx.tobytes() and d["full"][1].tobytes() == wn.tobytes()
    assert o.rebuildVoteStats() == vst and vst["scans"] == N_FRAMES and vst["rays_walked"] > 1000
    assert d["stats"] == dict(ast, voxels_after=want.size(), points_stored_after=want.pointCount())
    assert ast["voxels_after"] - vst["voxels_erased"] == want.size()
    never = drives["never"]
    record = dict(frames=N_FRAMES, params=VOTES, keyframe_voxels_without_votes=never["stats"]["voxels_after"],
                  ghost_points_without_votes=_ghosts(never["full"][0]), ghost_points_with_votes=_ghosts(d["full"][0]),
                  votes=vst)
    print("vote odometry record:", json.dumps(record))
    with open(os.path.join(ROOT, "profiles", "vote_odometry.json"), "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    for k in (N_FRAMES, N_FRAMES + 1):  # later frames go on aligning
        o.processCloud(_frame(k, True))
        s = o.stats
        assert s["initialised_keyframe"] == 0 and s["outer_iterations"] > 0
    # a failing vote is the rebuild's failure: the poses stay, the keyframe is left cleared
    p = o.getCurrentPose()
    before = p.translation.tobytes() + p.rotation.tobytes()
    far = d["poses"].copy()
    far[3, :3] = [0.0, -600000.0, 0.0]  # an origin out of range: the assembly culls that scan's points, the votes refuse it
    with pytest.raises(lom.LomError) as e:
        o.rebuildKeyframe(d["arch"], d["ids"], far, o.getCurrentPose())
    p = o.getCurrentPose()
    assert e.value.code == lom.capi.ERR_RANGE and p.translation.tobytes() + p.rotation.tobytes() == before
    assert len(o.getFullKeyFrameCloud()) == 0
