"""The grid shift (include/lidar_odometry_amd.h, "grid shift") restated: the shift of an array with a fill value, the two
rules of the geometry in Python float / numpy.float32, and the elevation record's cleared values.  A sequence is modelled
as: shift the arrays, then integrate at the new geometry (occupancy_ref.integrate(..., free=, seen=) and
elevation_ref.integrate(..., cells=) accept a starting state)."""
import math

import numpy as np

OK, ERR_ARG, ERR_RANGE = 0, -1, -3
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
MAX_SIDE = 16384
Q_LIMIT = 2 ** 40
# what lom_elevation_clear leaves in a cell, per array of lom_elevation_cells
ELEVATION_CLEARED = dict(count=0, zmin=I32_MAX, zmax=I32_MIN, sum=0)


def shift_array(a, dx, dy, fill):
    """out[iy, ix] = a[iy + dy, ix + dx] where that is in the array, else fill; a: (height, width)"""
    a = np.asarray(a)
    H, W = a.shape
    out = np.full_like(a, fill)
    x0, x1 = max(0, -dx), min(W, W - dx)   # the destination columns that have a source
    y0, y1 = max(0, -dy), min(H, H - dy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def kept_mask(W, H, dx, dy):
    """(height, width) bool: the destination cells that keep a source cell's content"""
    return shift_array(np.ones((H, W), bool), dx, dy, False)


def shift_elevation_cells(cells, dx, dy):
    return {k: shift_array(v, dx, dy, ELEVATION_CLEARED[k]) for k, v in cells.items()}


def _f32(v):
    return float(np.float32(v))


def geometry_ok(g):
    r, ox, oy = (np.float32(g[k]) for k in ("resolution", "origin_x", "origin_y"))
    return bool(np.isfinite(r) and r > 0 and np.isfinite(ox) and np.isfinite(oy) and 1 <= int(g["width"]) <= MAX_SIDE and
                1 <= int(g["height"]) <= MAX_SIDE)


def shifted_origin(origin, resolution, d):
    """(float)((double)origin + (double)d * (double)resolution), every operation rounded on its own; a numpy.float32"""
    with np.errstate(over="ignore"):
        return np.float32(_f32(origin) + float(int(d)) * _f32(resolution))


def shift_geometry(g, dx, dy):
    """(status, geometry or None): a dict like g (further keys, an elevation grid's z_ref, are carried) with numpy.float32
    origins"""
    if not geometry_ok(g):
        return ERR_ARG, None
    ox, oy = shifted_origin(g["origin_x"], g["resolution"], dx), shifted_origin(g["origin_y"], g["resolution"], dy)
    if not (np.isfinite(ox) and np.isfinite(oy)):
        return ERR_RANGE, None
    return OK, dict(g, origin_x=ox, origin_y=oy)


def geometry_bits(g):
    """the five fields as bytes: what same_geometry compares"""
    return (np.array([g["resolution"], g["origin_x"], g["origin_y"]], np.float32).tobytes() +
            np.array([g["width"], g["height"]], np.uint32).tobytes())


def cell_of(x, origin, resolution):
    """the grids' own index rule, in f64 from the f32 values; a float (it may be huge)"""
    return math.floor((float(x) - _f32(origin)) / _f32(resolution))


def follow_axis(x, origin, resolution, n, margin, quantum):
    """(status, d) of one axis"""
    qf = (float(x) - _f32(origin)) / _f32(resolution)
    if not math.isfinite(qf) or abs(math.floor(qf)) > Q_LIMIT:
        return ERR_RANGE, 0
    q = math.floor(qf)
    if margin <= q < n - margin:
        return OK, 0
    t = q - n // 2
    d = (abs(t) // quantum) * quantum * (1 if t >= 0 else -1)   # towards zero
    if abs(d) > I32_MAX:
        return ERR_RANGE, 0
    return OK, d


def follow_cells(q, n, margin, quantum):
    """the rule on the cell index itself, for an int64 array of q: the shifts d"""
    q = np.asarray(q, np.int64)
    t = q - n // 2
    d = np.sign(t) * ((np.abs(t) // quantum) * quantum)   # towards zero
    return np.where((q >= margin) & (q < n - margin), 0, d)


def follow(g, x, y, margin, quantum):
    """(status, dx, dy) of lom_grid_follow"""
    if not geometry_ok(g) or not (math.isfinite(x) and math.isfinite(y)) or quantum == 0:
        return ERR_ARG, 0, 0
    if margin + quantum > int(g["width"]) // 2 or margin + quantum > int(g["height"]) // 2:
        return ERR_ARG, 0, 0
    sx, dx = follow_axis(x, g["origin_x"], g["resolution"], int(g["width"]), margin, quantum)
    if sx != OK:
        return sx, 0, 0
    sy, dy = follow_axis(y, g["origin_y"], g["resolution"], int(g["height"]), margin, quantum)
    if sy != OK:
        return sy, 0, 0
    return OK, dx, dy
