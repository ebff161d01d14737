"""The clearance grid restated in numpy (include/lidar_odometry_amd.h, "clearance grid"): merge, distance, cost table,
cost, metres, summary and window.  The distance is restated separably -- the row distance by the index of the nearest
obstacle of the row, then the column minimum over 2R + 1 shifts -- which tests/test_clearance_host.py checks against a
brute-force all-pairs distance and against scipy's Euclidean distance transform.  Everything is integer except the cost
table, whose entries may differ from the library's by the last ulp of exp(): compare_table says how."""
import numpy as np

FAR = 65535
FREE_CLEARS_ELEVATION, UNKNOWN_IS_OBSTACLE = 1, 2
MAX_R = 254
SUMMARY_KEYS = ("cells_lethal", "cells_inscribed", "cells_costed", "cells_unknown", "cells_invalid", "cells_cleared")


def geometry(resolution, origin_x, origin_y, width, height):
    return dict(resolution=np.float32(resolution), origin_x=np.float32(origin_x), origin_y=np.float32(origin_y),
                width=int(width), height=int(height))


def params(inflation_radius, inscribed_radius, decay, flags=0):
    return dict(inflation_radius=np.float32(inflation_radius), inscribed_radius=np.float32(inscribed_radius),
                decay=np.float32(decay), flags=int(flags))


def radius_cells(p, resolution):
    """R, or None where the library refuses"""
    q = np.floor(np.float64(np.float32(p["inflation_radius"])) / np.float64(np.float32(resolution)))
    return int(q) if 0 <= q <= MAX_R else None


def params_ok(p, resolution):
    v = [np.float32(p[k]) for k in ("inflation_radius", "inscribed_radius", "decay")]
    return bool(all(np.isfinite(v)) and 0 <= v[1] <= v[0] and v[2] >= 0 and not (p["flags"] & ~3)
                and radius_cells(p, resolution) is not None)


def cost_table(p, resolution):
    """step 3: uint8, R^2 + 1 entries"""
    R = radius_cells(p, resolution)
    r, ins, inf, decay = (np.float64(np.float32(v)) for v in (resolution, p["inscribed_radius"], p["inflation_radius"], p["decay"]))
    dist = np.sqrt(np.arange(R * R + 1, dtype=np.float64)) * r
    t = np.floor(98.0 * np.exp(-decay * (dist - ins)))
    t = np.where(dist > inf, 0.0, t)
    t = np.where(dist <= ins, 99.0, t)
    t[0] = 100.0
    return t.astype(np.uint8)


def compare_table(got, p, resolution):
    """the library's table against step 3: exactly 100 / 99 / 0 at k = 0, dist <= inscribed, dist > inflation; elsewhere
    equal or off by one (the last ulp of exp); non-increasing in k"""
    want = cost_table(p, resolution)
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.shape, want.shape)
    fixed = (want == 100) | (want == 99)
    r, inf = np.float64(np.float32(resolution)), np.float64(np.float32(p["inflation_radius"]))
    fixed |= np.sqrt(np.arange(len(want), dtype=np.float64)) * r > inf
    assert np.array_equal(got[fixed], want[fixed])
    assert (np.abs(got.astype(int) - want.astype(int)) <= 1).all() and (got[~fixed] <= 98).all()
    assert (np.diff(got.astype(int)) <= 0).all()


def merge(occ, elev, flags, shape=None):
    """step 1: (base int8, obstacle bool, invalid bool, cleared bool)"""
    shape = shape or (occ if occ is not None else elev).shape
    o = np.full(shape, -1, int) if occ is None else np.asarray(occ, np.int8).astype(int)
    e = np.full(shape, -1, int) if elev is None else np.asarray(elev, np.int8).astype(int)
    bad_o, bad_e = ~np.isin(o, (-1, 0, 100)), (e < -1) | (e > 100)
    o, e = np.where(bad_o, -1, o), np.where(bad_e, -1, e)
    cleared = (e == 100) & bool(flags & FREE_CLEARS_ELEVATION) & (o == 0)
    e = np.where(cleared, 0, e)
    base = np.where((o == 100) | (e == 100), 100, np.where(e >= 0, e, np.where(o == 0, 0, -1)))
    obstacle = (base == 100) | ((base == -1) & bool(flags & UNKNOWN_IS_OBSTACLE))
    return base.astype(np.int8), obstacle, bad_o | bad_e, cleared


def row_distance(ob, R):
    """g: per cell, the distance along its row to the nearest obstacle of the row, clipped to R + 1"""
    h, w = ob.shape
    idx = np.arange(w)[None, :]
    big = 4 * (w + R + 2)
    left = np.maximum.accumulate(np.where(ob, idx, -big), axis=1)                       # index of the nearest at or left
    right = np.minimum.accumulate(np.where(ob, idx, big)[:, ::-1], axis=1)[:, ::-1]     # ... at or right
    return np.minimum(np.minimum(idx - left, right - idx), R + 1).astype(np.int64)


def distance_sq(ob, R):
    """step 2: uint16, the squared distance in cells to the nearest obstacle if <= R^2, else FAR"""
    h, w = ob.shape
    g = row_distance(ob, R)
    pad = np.full((R, w), R + 1, np.int64)
    gp = np.concatenate([pad, g, pad])
    best = np.full((h, w), (R + 1) ** 2 + R * R, np.int64)
    for dy in range(-R, R + 1):
        best = np.minimum(best, gp[R + dy:R + dy + h] ** 2 + dy * dy)
    return np.where(best <= R * R, best, FAR).astype(np.uint16)


def brute_distance_sq(ob, R):
    """the same by all pairs (small grids)"""
    h, w = ob.shape
    ys, xs = np.nonzero(ob)
    Y, X = np.mgrid[0:h, 0:w]
    if not len(ys):
        return np.full((h, w), FAR, np.uint16)
    d = ((Y[..., None] - ys) ** 2 + (X[..., None] - xs) ** 2).min(axis=-1)
    return np.where(d <= R * R, d, FAR).astype(np.uint16)


def cost_of(base, d2, table):
    """step 4"""
    far = d2 == FAR
    c = np.where(far, 0, table[np.where(far, 0, d2)]).astype(int)
    b = base.astype(int)
    return np.where(d2 == 0, 100, np.where(b >= 0, np.maximum(b, c), np.where(c > 0, c, -1))).astype(np.int8)


def metres(d2, resolution):
    """step 5, float32"""
    with np.errstate(invalid="ignore"):
        m = np.sqrt(d2.astype(np.float64)) * np.float64(np.float32(resolution))
    return np.where(d2 == FAR, np.inf, m).astype(np.float32)


def clip(window, geo):
    """(x0, y0, x1, y1) of the window (x0, y0, width, height; None: the grid) clipped to the grid, or None if empty"""
    if window is None:
        return 0, 0, geo["width"], geo["height"]
    x0, y0 = max(int(window[0]), 0), max(int(window[1]), 0)
    x1, y1 = min(int(window[0]) + int(window[2]), geo["width"]), min(int(window[1]) + int(window[3]), geo["height"])
    return None if x0 >= x1 or y0 >= y1 else (x0, y0, x1, y1)


def empty_state(geo):
    shape = (geo["height"], geo["width"])
    return dict(d2=np.full(shape, FAR, np.uint16), cost=np.full(shape, -1, np.int8))


def update(geo, occ, elev, p, window=None, state=None, table=None):
    """an update: dict(d2, cost, summary, error).  `state`: the planes before (default: after create); they are not
    written to.  `table`: the library's cost table, for a comparison of the cost byte by byte (default: cost_table)."""
    state = state or empty_state(geo)
    zero = dict.fromkeys(SUMMARY_KEYS, 0)
    if (occ is None and elev is None) or not params_ok(p, geo["resolution"]):
        return dict(d2=state["d2"], cost=state["cost"], summary=zero, error=True)
    rect = clip(window, geo)
    if rect is None:
        return dict(d2=state["d2"], cost=state["cost"], summary=zero, error=False)
    R = radius_cells(p, geo["resolution"])
    table = cost_table(p, geo["resolution"]) if table is None else table
    base, ob, invalid, cleared = merge(occ, elev, p["flags"], (geo["height"], geo["width"]))
    d2_full = distance_sq(ob, R)
    cost_full = cost_of(base, d2_full, table)
    x0, y0, x1, y1 = rect
    d2, cost = state["d2"].copy(), state["cost"].copy()
    d2[y0:y1, x0:x1], cost[y0:y1, x0:x1] = d2_full[y0:y1, x0:x1], cost_full[y0:y1, x0:x1]
    c = cost[y0:y1, x0:x1]
    summary = dict(cells_lethal=int((c == 100).sum()), cells_inscribed=int((c == 99).sum()),
                   cells_costed=int(((c >= 0) & (c < 99)).sum()), cells_unknown=int((c < 0).sum()),
                   cells_invalid=int(invalid[y0:y1, x0:x1].sum()), cells_cleared=int(cleared[y0:y1, x0:x1].sum()))
    return dict(d2=d2, cost=cost, summary=summary, error=False)


def plane_summary(cost):
    """what lom_clearance_cost reports of a whole plane"""
    return dict(cells_lethal=int((cost == 100).sum()), cells_inscribed=int((cost == 99).sum()),
                cells_costed=int(((cost >= 0) & (cost < 99)).sum()), cells_unknown=int((cost < 0).sum()), cells_invalid=0,
                cells_cleared=0)


def query(geo, d2, cost, xy):
    """(metres float32, cost int8) of the cells of the points; NaN and -1 outside"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    r = np.float64(geo["resolution"])
    with np.errstate(invalid="ignore"):
        qx = np.floor((xy[:, 0] - np.float64(geo["origin_x"])) / r)
        qy = np.floor((xy[:, 1] - np.float64(geo["origin_y"])) / r)
        inside = (qx >= 0) & (qx < geo["width"]) & (qy >= 0) & (qy < geo["height"])
    ix, iy = np.where(inside, qx, 0).astype(int), np.where(inside, qy, 0).astype(int)
    m = metres(d2, geo["resolution"])
    return np.where(inside, m[iy, ix], np.float32(np.nan)).astype(np.float32), np.where(inside, cost[iy, ix], -1).astype(np.int8)
