"""Reference of the elevation grid (include/lidar_odometry_amd.h, "elevation grid"): the definition restated in numpy f64
from the header's text, every operation rounded on its own.  The transform is assemble_ref's and the hit rule is
occupancy_ref.rays'; the height quantisation, the integer accumulators, the int64 plane fit by Cramer's rule, the layers
and the cost are written here.  The integer sums are numpy int64, with an assertion that every numerator stays below 2^53."""
import numpy as np

from tests import assemble_ref as A
from tests import occupancy_ref as O

Q = 2.0 ** -8
H_LIMIT = 2048.0
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
UNKNOWN, LETHAL = -1, 100
LAYERS = ("min", "max", "mean", "slope", "rough", "step")


def geometry(resolution, origin_x, origin_y, width, height, z_ref):
    return dict(resolution=resolution, origin_x=origin_x, origin_y=origin_y, width=width, height=height, z_ref=z_ref)


def point_params(z_lo, z_hi, min_range, max_range):
    return dict(z_lo=z_lo, z_hi=z_hi, min_range=min_range, max_range=max_range)


def layer_params(min_points, window):
    return dict(min_points=min_points, window=window)


def cost_params(max_slope, max_step, max_rough, max_span):
    return dict(max_slope=max_slope, max_step=max_step, max_rough=max_rough, max_span=max_span)


def _f(v):
    """an f32 value widened"""
    return float(np.float32(v))


def empty_cells(geo):
    H, W = int(geo["height"]), int(geo["width"])
    return dict(count=np.zeros((H, W), np.uint32), zmin=np.full((H, W), I32_MAX, np.int32),
                zmax=np.full((H, W), I32_MIN, np.int32), sum=np.zeros((H, W), np.int64))


def scan_points(geo, pose, xyz, p):
    """One scan at its pose: (cell (m, 2) int64 as x, y; zq (m,) int64) of the contributing points in input order, and the
    number of hits out of the height range"""
    x, _ = A.transform(pose, xyz, np.zeros_like(np.asarray(xyz, np.float32).reshape(-1, 3)))
    R = O.rays(geo, O.origin_of(pose), x, dict(p, margin=0.0))
    hit = R["hit"]
    with np.errstate(all="ignore"):
        h = x[:, 2].astype(np.float64) - _f(geo["z_ref"])
        inside = np.abs(h) < H_LIMIT
        zq = np.rint(h * 256.0)  # ties to even
    use = hit & inside
    return R["hit_cell"][use], zq[use].astype(np.int64), int((hit & ~inside).sum())


def integrate(geo, scans, ids, poses, p, cells=None):
    """dict(error: the LOM_ERR_RANGE verdict; cells: dict(count, zmin, zmax, sum), accumulated onto the ones given (which
    are left unchanged); stats as lom_elevation_stats).  scans: list of xyz (or of (xyz, nrm): normals are ignored)"""
    W = int(geo["width"])
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    cells = empty_cells(geo) if cells is None else {k: np.array(v) for k, v in cells.items()}
    out = dict(error=False, cells=cells, stats=None)
    for k in range(len(ids)):  # the verdict comes before anything changes (an origin counts even for an empty scan)
        if not O.start_cell(geo, O.origin_of(poses[k]))[2]:
            out["error"] = True
            return out
    count = cells["count"].astype(np.int64).ravel()
    zmin, zmax, total = cells["zmin"].astype(np.int64).ravel(), cells["zmax"].astype(np.int64).ravel(), cells["sum"].ravel()
    was_empty = count == 0
    st = dict(scans=len(ids), points=0, points_marked=0, points_out_of_height=0, cells_new=0)
    for k, i in enumerate(ids):
        xyz = scans[int(i)]
        if isinstance(xyz, tuple):
            xyz = xyz[0]
        c, zq, n_out = scan_points(geo, poses[k], xyz, p)
        flat = c[:, 1] * W + c[:, 0]
        np.add.at(count, flat, 1)
        np.minimum.at(zmin, flat, zq)
        np.maximum.at(zmax, flat, zq)
        np.add.at(total, flat, zq)
        st["points"] += len(np.asarray(xyz).reshape(-1, 3))
        st["points_marked"] += len(zq)
        st["points_out_of_height"] += n_out
    st["cells_new"] = int((was_empty & (count > 0)).sum())
    shape = cells["count"].shape
    assert count.max(initial=0) < 2 ** 32
    out.update(cells=dict(count=count.astype(np.uint32).reshape(shape), zmin=zmin.astype(np.int32).reshape(shape),
                          zmax=zmax.astype(np.int32).reshape(shape), sum=total.reshape(shape)), stats=st)
    return out


def _window(valid, zmin, R):
    """yields (i, j, v, d) over the window in row-major order: v = the cell (x + i, y + j) is valid and in the grid (and
    the centre is valid), d = its zmin minus the centre's where v, else 0 (int64)"""
    H, W = valid.shape
    vp = np.zeros((H + 2 * R, W + 2 * R), bool)
    zp = np.zeros((H + 2 * R, W + 2 * R), np.int64)
    vp[R:R + H, R:R + W], zp[R:R + H, R:R + W] = valid, zmin
    z0 = zmin.astype(np.int64)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            v = vp[R + j:R + j + H, R + i:R + i + W] & valid
            d = np.where(v, zp[R + j:R + j + H, R + i:R + i + W] - z0, 0)
            yield i, j, v, d


def derive(geo, cells, lp):
    """The header's steps 1 to 6 for every cell, in f64: dict(valid, det, slope, rough, step, span, min, max, mean);
    slope and rough are NaN where det == 0; everything is only meaningful where valid"""
    R, min_points = int(lp["window"]), int(lp["min_points"])
    count, zmin = cells["count"].astype(np.int64), cells["zmin"].astype(np.int64)
    valid = count >= min_points
    zero = np.zeros(valid.shape, np.int64)
    n, Si, Sj, Sii, Sij, Sjj, Sd, Sid, Sjd, step_q = (zero.copy() for _ in range(10))
    for i, j, v, d in _window(valid, zmin, R):
        n += v
        Si += v * i
        Sj += v * j
        Sii += v * (i * i)
        Sij += v * (i * j)
        Sjj += v * (j * j)
        Sd += d
        Sid += i * d
        Sjd += j * d
        if abs(i) <= 1 and abs(j) <= 1 and (i or j):
            step_q = np.maximum(step_q, np.abs(d))
    det = Sii * (Sjj * n - Sj * Sj) - Sij * (Sij * n - Sj * Si) + Si * (Sij * Sj - Sjj * Si)
    a_num = Sid * (Sjj * n - Sj * Sj) - Sij * (Sjd * n - Sj * Sd) + Si * (Sjd * Sj - Sjj * Sd)
    b_num = Sii * (Sjd * n - Sj * Sd) - Sid * (Sij * n - Sj * Si) + Si * (Sij * Sd - Sjd * Si)
    c_num = Sii * (Sjj * Sd - Sjd * Sj) - Sij * (Sij * Sd - Sjd * Si) + Sid * (Sij * Sj - Sjj * Si)
    for num in (det, a_num, b_num, c_num):
        assert np.abs(num).max(initial=0) < 2 ** 53, "a Cramer numerator left the exact range of f64"
    assert (det >= 0).all()
    pos = valid & (det > 0)
    r = _f(geo["resolution"])
    with np.errstate(all="ignore"):
        fd = det.astype(np.float64)
        Af, Bf, Cf = a_num.astype(np.float64) / fd, b_num.astype(np.float64) / fd, c_num.astype(np.float64) / fd
        slope = (np.sqrt(Af * Af + Bf * Bf) * Q) / r
        S = np.zeros(valid.shape, np.float64)
        for i, j, v, d in _window(valid, zmin, R):
            e = d.astype(np.float64) - ((Af * float(i) + Bf * float(j)) + Cf)
            S = np.where(v & pos, S + e * e, S)
        rough = np.sqrt(S / n.astype(np.float64)) * Q
        z_ref = _f(geo["z_ref"])
        mean = z_ref + (cells["sum"].astype(np.float64) * Q) / count.astype(np.float64)
    return dict(valid=valid, det=det, slope=np.where(pos, slope, np.nan), rough=np.where(pos, rough, np.nan),
                step=Q * step_q.astype(np.float64), span=Q * (cells["zmax"].astype(np.int64) - zmin).astype(np.float64),
                min=z_ref + zmin.astype(np.float64) * Q, max=z_ref + cells["zmax"].astype(np.float64) * Q, mean=mean)


def layers(geo, cells, lp):
    """dict of the six float32 layers, NaN where a cell is invalid"""
    d = derive(geo, cells, lp)
    with np.errstate(all="ignore"):
        return {k: np.where(d["valid"], d[k], np.nan).astype(np.float32) for k in LAYERS}


def cost(geo, cells, lp, cp):
    """(int8 grid, summary as lom_elevation_summary, dict of what the branches saw: for the tests' coverage checks)"""
    d = derive(geo, cells, lp)
    ms, mt, mr, mp = (_f(cp[k]) for k in ("max_slope", "max_step", "max_rough", "max_span"))
    valid, pos = d["valid"], d["valid"] & (d["det"] > 0)
    with np.errstate(all="ignore"):
        lethal = valid & ((d["span"] > mp) | (d["step"] > mt) | (pos & (d["slope"] > ms)))
        m = np.maximum(d["step"] / mt, np.maximum(np.where(pos, d["slope"] / ms, 0.0), np.where(pos, d["rough"] / mr, 0.0)))
        c = np.floor(99.0 * np.minimum(m, 1.0))
    c = np.where(valid, c, 0.0)
    out = np.where(~valid, UNKNOWN, np.where(lethal, LETHAL, c)).astype(np.int8)
    summary = dict(cells_unknown=int((~valid).sum()), cells_lethal=int(lethal.sum()), cells_costed=int((valid & ~lethal).sum()))
    seen = dict(lethal_span=valid & (d["span"] > mp), lethal_step=valid & (d["step"] > mt), lethal_slope=pos & (d["slope"] > ms),
                m_is_one=valid & ~lethal & (m == 1.0), m_above_one=valid & ~lethal & (m > 1.0), flat_fit=valid & ~pos)
    return out, summary, seen
