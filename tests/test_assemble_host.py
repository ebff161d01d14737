"""Scan archive and map assembly without a GPU: the rotation matrix of tests/assemble_ref.py against the library's byte for
byte, the ABI, and every refusal that comes before device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import assemble_ref as ref
from tests.conftest import ROOT

SYMBOLS = ["lom_archive_create", "lom_archive_destroy", "lom_archive_last_error", "lom_archive_clear", "lom_archive_stream",
           "lom_archive_device", "lom_archive_wait_event", "lom_archive_add", "lom_archive_add_device",
           "lom_archive_scan_count", "lom_archive_point_count", "lom_archive_scan_size", "lom_archive_get",
           "lom_map_assemble", "lom_odometry_archive_scan", "lom_odometry_rebuild_keyframe"]


def test_rotation_matrix_equals_the_library_byte_for_byte(lom):
    rng = np.random.default_rng(7)
    poses = np.zeros((400, 7))
    poses[:, :3] = rng.normal(size=(400, 3)) * 100.0
    q = rng.normal(size=(400, 4))
    q[:100] /= np.linalg.norm(q[:100], axis=1)[:, None]  # (nearly) unit; the rest unnormalised, tiny and huge among them
    q[100:150] *= 1e-12
    q[150:200] *= 1e9
    q[::2, 0] = -np.abs(q[::2, 0])  # w < 0
    q[-1] = [1.0, 0.0, 0.0, 0.0]
    q[-2] = [0.0, 0.0, 0.0, -3.0]
    poses[:, 3:] = q
    for p in poses:
        assert lom.graph_pose_rotation_matrix(p).tobytes() == ref.rotation_matrix(p).tobytes()
    R = lom.graph_pose_rotation_matrix(poses[0])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
    assert np.array_equal(lom.graph_pose_rotation_matrix(poses[-1]), np.eye(3))


def test_rotation_matrix_refusals(lom):
    L, E = lom.capi.lib(), lom.capi.ERR_ARG
    out = np.zeros(9)
    pose = np.zeros(1, lom.capi.GRAPH_POSE)
    assert L.lom_graph_pose_rotation_matrix(pose.ctypes.data, out.ctypes.data) == E  # zero quaternion
    pose["q_wxyz"][0, 0] = 1.0
    assert L.lom_graph_pose_rotation_matrix(None, out.ctypes.data) == E
    assert L.lom_graph_pose_rotation_matrix(pose.ctypes.data, None) == E
    assert L.lom_graph_pose_rotation_matrix(pose.ctypes.data, out.ctypes.data) == 0
    for field, k in (("t", 1), ("q_wxyz", 2)):
        for bad in (np.nan, np.inf):
            p = pose.copy()
            p[field][0, k] = bad
            assert L.lom_graph_pose_rotation_matrix(p.ctypes.data, out.ctypes.data) == E
    with pytest.raises(lom.LomError):
        lom.graph_pose_rotation_matrix(np.zeros(7))


def test_f64_poses_carry_weight_in_the_reference():
    """the far translation the GPU test uses: rounding the pose to f32 first changes output bits"""
    pose = np.array([1234.56789, -987.654321, 12.3456789, 0.9, 0.1, -0.3, 0.2])
    rounded = pose.astype(np.float32).astype(np.float64)
    xyz = np.random.default_rng(3).normal(size=(257, 3)).astype(np.float32) * 20
    a, an = ref.transform(pose, xyz, xyz)
    b, bn = ref.transform(rounded, xyz, xyz)
    assert (a.view(np.uint32) != b.view(np.uint32)).any()


def test_symbols_declared_exported_and_sized(lom):
    hdr = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    assert re.search(r"scan archive and map assembly", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = lom.capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in lom.capi.EXPORTED and hasattr(L, name), name
    assert sorted(set(re.findall(r"\b(lom_archive_[a-z0-9_]+)\s*\(", code))) == sorted(s for s in SYMBOLS if "_archive_" in s and "odometry" not in s)
    assert re.search(r"\blom_graph_pose_rotation_matrix\s*;", code)
    assert lom.capi.EXPORTED_BY_TYPE == ["lom_graph_pose_rotation_matrix"] and hasattr(L, "lom_graph_pose_rotation_matrix")
    assert C.sizeof(lom.capi.AssembleParams) == 16 and C.sizeof(lom.capi.AssembleStats) == 48
    assert lom.capi.AssembleParams.radius.offset == 12 and lom.capi.AssembleStats.points_stored_after.offset == 40
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for word in ("class ScanArchive", "assemble(", "archiveScan(", "rebuildKeyframe("):
        assert word in mirror, word
    assert L.lom_abi_version() == 2


def test_null_and_bad_arguments_are_refused_without_a_device(lom):
    L, E = lom.capi.lib(), lom.capi.ERR_ARG
    h = C.c_void_p()
    assert L.lom_archive_create(0, 4, 4, None) == E
    assert L.lom_archive_create(0, (1 << 32) + 1, 4, C.byref(h)) == E and not h.value
    assert L.lom_archive_create(0, 4, (1 << 24) + 1, C.byref(h)) == E and not h.value
    xyz = np.zeros((2, 3), np.float32)
    pose = np.zeros(1, lom.capi.GRAPH_POSE)
    pose["q_wxyz"][0, 0] = 1.0
    ids = np.zeros(1, np.int64)
    st, id_ = lom.capi.AssembleStats(), C.c_int64()
    cur = lom.capi.Pose(lom.capi.f3((0, 0, 0)), lom.capi.f4((1, 0, 0, 0)))
    assert L.lom_archive_clear(None) == E and L.lom_archive_device(None) == E and L.lom_archive_stream(None) is None
    assert L.lom_archive_wait_event(None, None) == E
    assert L.lom_archive_add(None, xyz.ctypes.data, xyz.ctypes.data, 2, 12) == E
    assert L.lom_archive_add_device(None, xyz.ctypes.data, xyz.ctypes.data, 2, 12, None) == E
    assert L.lom_archive_scan_count(None) == E and L.lom_archive_point_count(None) == E
    assert L.lom_archive_scan_size(None, 0) == E and L.lom_archive_get(None, 0, None, None, 0) == E
    assert L.lom_map_assemble(None, None, ids.ctypes.data, pose.ctypes.data, 1, None, C.byref(st)) == E
    assert L.lom_odometry_archive_scan(None, None, C.byref(id_)) == E
    assert L.lom_odometry_rebuild_keyframe(None, None, ids.ctypes.data, pose.ctypes.data, 1, C.byref(cur), None) == E
    L.lom_archive_destroy(None)
    assert L.lom_archive_last_error(None) is not None
    if L.lom_device_count() < 1:  # a host without a device: a loud failure, no fallback
        with pytest.raises(lom.LomError) as e:
            lom.ScanArchive()
        assert e.value.code == lom.capi.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
