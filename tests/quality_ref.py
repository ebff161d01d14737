"""Reference side of the quality-report tests (test infrastructure): the values beyond the align's 28 sums restated in
numpy from the oracle's correspondences, the host math restated with numpy.linalg, and the scenes the tests share.

`R p` is the rotation as the reference's Evaluate applies it to a quaternion that need not be a unit one
(oracle/oracle.c quat_rotate_d): p + w (2 u x p) + u x (2 u x p), in f64."""
import ctypes as C

import numpy as np

HUBER_A = 0.15
DBL_MIN = np.finfo(np.float64).tiny

# lom_quality_report: (field, offset, bytes)
REPORT_LAYOUT = [
    ("queries", 0, 8), ("valid", 8, 8), ("inliers", 16, 8), ("overlap", 24, 8), ("cost", 32, 8), ("rmse", 40, 8),
    ("rmse_inliers", 48, 8), ("max_abs_residual", 56, 8), ("mean_sq_dist", 64, 8), ("sigma2", 72, 8), ("sum_w", 80, 8),
    ("information", 88, 288), ("gradient", 376, 48), ("eig_t", 424, 24), ("eigvec_t", 448, 72), ("eig_r", 520, 24),
    ("eigvec_r", 544, 72), ("covariance", 616, 288), ("degenerate_t", 904, 4), ("degenerate_r", 908, 4),
    ("covariance_valid", 912, 4), ("pad", 916, 4),
]
REPORT_SIZE = 920


def rotate(q, p):
    w, u = q[0], np.asarray(q[1:], np.float64)
    uv = 2.0 * np.cross(u, p)
    return p + w * uv + np.cross(u, uv)


def residuals_from_pairs(pairs, scan, q, t):
    """(valid mask, signed residuals r = (R p + t - o).n, squared point-to-point distances |R p + t - o|^2), f64, in
    scan order; entries without a pair are NaN."""
    valid = pairs["index"] >= 0
    p = np.asarray(scan, np.float64)
    e = rotate(np.asarray(q, np.float64), p) + np.asarray(t, np.float64) - pairs["origin"].astype(np.float64)
    n = pairs["normal"].astype(np.float64)
    r = e[:, 0] * n[:, 0] + (e[:, 1] * n[:, 1] + e[:, 2] * n[:, 2])
    d2 = e[:, 0] * e[:, 0] + (e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
    r[~valid] = np.nan
    d2[~valid] = np.nan
    return valid, r, d2


def extra_sums(valid, r, d2):
    """sums [28..35] of LOM_NQSUMS from the per-point residuals."""
    rv, dv = r[valid], d2[valid]
    s = rv * rv
    inl = s <= HUBER_A * HUBER_A
    w = np.ones_like(s)
    w[~inl] = np.maximum(DBL_MIN, HUBER_A / np.sqrt(s[~inl]))
    return np.array([w.sum(), (w * s).sum(), s.sum(), s[inl].sum(), dv.sum(), float(valid.sum()), float(inl.sum()),
                     np.abs(rv).max() if len(rv) else 0.0], np.float64)


def sums36(sums28, extras):
    out = np.zeros(36, np.float64)
    out[:28] = np.asarray(sums28, np.float64)[:28]
    out[28:] = extras
    return out


def full_information(sums):
    H = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = sums[k]
            k += 1
    return H


def nav_information(H):
    """S P H P^T S: translation first, the half-angle tangent rescaled to radians."""
    perm = [3, 4, 5, 0, 1, 2]
    s = np.array([1, 1, 1, 0.5, 0.5, 0.5])
    return H[np.ix_(perm, perm)] * np.outer(s, s)


def from_sums(lom, sums, queries, min_eig_t=0.0, min_eig_r=0.0):
    rep = lom.capi.QualityReport()
    arr = (C.c_double * 36)(*[float(v) for v in sums])
    rc = lom.capi.lib().lom_quality_from_sums(arr, int(queries), float(min_eig_t), float(min_eig_r), C.byref(rep))
    assert rc == 0, rc
    return rep.asdict()


def _grid(a, b, step):
    return np.arange(a, b + 0.5 * step, step)


def corridor_scene(end_wall=False):
    """Floor z = 0 and walls y = +-2 along x, exact axis normals; with `end_wall` also the wall x = 10 (a corner: every
    direction constrained).  Returns (map xyz, map normals, scan = every third map point)."""
    xs = _grid(-10.0, 9.75, 0.25)
    fy = _grid(-1.75, 1.75, 0.25)
    wz = _grid(0.25, 3.0, 0.25)
    fx, fyy = np.meshgrid(xs, fy, indexing="ij")
    floor = np.c_[fx.ravel(), fyy.ravel(), np.zeros(fx.size)]
    wx, wzz = np.meshgrid(xs, wz, indexing="ij")
    wall_l = np.c_[wx.ravel(), np.full(wx.size, 2.0), wzz.ravel()]
    wall_r = np.c_[wx.ravel(), np.full(wx.size, -2.0), wzz.ravel()]
    pts = [floor, wall_l, wall_r]
    nrm = [np.tile([0.0, 0.0, 1.0], (len(floor), 1)), np.tile([0.0, -1.0, 0.0], (len(wall_l), 1)),
           np.tile([0.0, 1.0, 0.0], (len(wall_r), 1))]
    if end_wall:
        ey, ez = np.meshgrid(fy, wz, indexing="ij")
        end = np.c_[np.full(ey.size, 10.0), ey.ravel(), ez.ravel()]
        pts.append(end)
        nrm.append(np.tile([-1.0, 0.0, 0.0], (len(end), 1)))
    xyz = np.concatenate(pts).astype(np.float32)
    n = np.concatenate(nrm).astype(np.float32)
    return xyz, n, np.ascontiguousarray(xyz[::3])
