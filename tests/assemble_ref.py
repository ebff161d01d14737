"""The map assembly of include/lidar_odometry_amd.h ("scan archive and map assembly") restated in numpy f64, operation by
operation: quaternion to R, the transform, the cull.  Every line rounds on its own, as the header asks; the results are
compared with the library's byte for byte.  The reference MAP is then the library's own, oracle-pinned insert: a second
VoxelGrid and one addCloud of what concatenated() returns."""
import numpy as np


def rotation_matrix(pose):
    """pose: 7 float64 (t, then q wxyz).  The header's formula from the quaternion normalised as lom_graph_add_node does."""
    q = np.asarray(pose, np.float64)[3:7]
    n2 = np.float64(0.0)
    for a in range(4):
        n2 = n2 + q[a] * q[a]
    w, x, y, z = (q[a] / np.sqrt(n2) for a in range(4))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]], np.float64)


def transform(pose, xyz, nrm):
    """x' = (f32)((R0 p0 + (R1 p1 + R2 p2)) + t0) in f64; the normal likewise without t"""
    R = rotation_matrix(pose)
    t = np.asarray(pose, np.float64)[:3]
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    n = np.asarray(nrm, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.empty((len(p), 3), np.float32)
    out_n = np.empty((len(p), 3), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((R[r, 0] * p[:, 0] + (R[r, 1] * p[:, 1] + R[r, 2] * p[:, 2])) + t[r]).astype(np.float32)
            out_n[:, r] = (R[r, 0] * n[:, 0] + (R[r, 1] * n[:, 1] + R[r, 2] * n[:, 2])).astype(np.float32)
    return out, out_n


def kept(xyz, centre, radius):
    """the cull on the f32 result: dropped iff dx dx + (dy dy + dz dz) > radius radius, f32, strict"""
    if centre is None or not radius > 0.0:
        return np.ones(len(xyz), bool)
    c = np.asarray(centre, np.float32)
    r = np.float32(radius)
    with np.errstate(all="ignore"):
        d = xyz - c[None, :]
        d2 = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        assert d2.dtype == np.float32
        return ~(d2 > r * r)


def concatenated(scans, ids, poses, centre=None, radius=0.0):
    """scans: list of (xyz, nrm); the concatenated f32 cloud C, Cn of the header's contract"""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    xs, ns = [np.empty((0, 3), np.float32)], [np.empty((0, 3), np.float32)]
    for k, i in enumerate(ids):
        x, n = transform(poses[k], *scans[int(i)])
        keep = kept(x, centre, radius)
        xs.append(x[keep])
        ns.append(n[keep])
    return np.concatenate(xs), np.concatenate(ns)
