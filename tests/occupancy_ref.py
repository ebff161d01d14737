"""Reference of the occupancy grid (include/lidar_odometry_amd.h, "occupancy grid"): the definition restated in numpy f64
from the header's text, every operation rounded on its own.  The transform is assemble_ref's; the index rule (floor, in
f64, compared before any conversion), the ray, the hit, the walk, the votes and the classification are written here."""
import math

import numpy as np

from tests import assemble_ref as A

CELL_LIMIT = 1 << 30
FREE, OCCUPIED, UNKNOWN = 0, 100, -1


def geometry(resolution, origin_x, origin_y, width, height):
    return dict(resolution=resolution, origin_x=origin_x, origin_y=origin_y, width=width, height=height)


def ray_params(z_lo, z_hi, margin, min_range, max_range):
    return dict(z_lo=z_lo, z_hi=z_hi, margin=margin, min_range=min_range, max_range=max_range)


def rule(min_free_scans, free_per_seen, min_seen_scans):
    return dict(min_free_scans=min_free_scans, free_per_seen=free_per_seen, min_seen_scans=min_seen_scans)


def _f(v):
    """an f32 value widened"""
    return float(np.float32(v))


def max_steps(max_range, resolution):
    return 2 * (math.ceil(_f(max_range) / _f(resolution)) + 2)


def origin_of(pose):
    """step 2: the pose's translation, each component rounded to f32"""
    with np.errstate(all="ignore"):
        return np.asarray(pose, np.float64)[:3].astype(np.float32)


def start_cell(geo, origin32):
    """(O2 (2,), c (2,) float: floor(O2_a / r), ok: |c_a| < 2^30 on both axes and finite)"""
    r = _f(geo["resolution"])
    G = np.array([_f(geo["origin_x"]), _f(geo["origin_y"])])
    with np.errstate(all="ignore"):
        O2 = np.asarray(origin32, np.float32).astype(np.float64)[:2] - G
        c = np.floor(O2 / r)
    ok = bool(np.all(np.isfinite(c)) and np.all(np.abs(c) < CELL_LIMIT))
    return O2, c, ok


def _t_of(c, s, O2, D, r):
    """t_a = ((double)b_a r - O2_a) / D_a with b_a = s_a > 0 ? c_a + 1 : c_a; +inf where D_a == 0"""
    b = np.where(s > 0, c + 1, c).astype(np.float64)
    with np.errstate(all="ignore"):
        t = (b * r - O2) / D
    return np.where(D == 0, np.inf, t)


def rays(geo, origin32, pts32, p):
    """steps 3 and 4 per ray: dict(D (n, 3), t_end, walked, hit (bool), hit_cell (n, 2) int64, valid where hit)"""
    r = _f(geo["resolution"])
    G = np.array([_f(geo["origin_x"]), _f(geo["origin_y"])])
    W, H = int(geo["width"]), int(geo["height"])
    z_lo, z_hi, margin, min_range, max_range = (_f(p[k]) for k in ("z_lo", "z_hi", "margin", "min_range", "max_range"))
    O = np.asarray(origin32, np.float32).astype(np.float64).reshape(3)
    P = np.asarray(pts32, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        D = P - O
        L = np.sqrt(D[:, 0] * D[:, 0] + (D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2]))
        Dz = D[:, 2]
        t_band = np.where(Dz > 0, z_hi / Dz, np.where(Dz < 0, z_lo / Dz, np.inf))
        reach = np.where(L < max_range, L, max_range) - margin
        q = reach / L
        t_end = np.where(q < t_band, q, t_band)
        walked = (L >= min_range) & (t_end > 0)
        hq = np.floor((P[:, :2] - G) / r)
        in_grid = (hq[:, 0] >= 0) & (hq[:, 0] < W) & (hq[:, 1] >= 0) & (hq[:, 1] < H)
        hit = (L >= min_range) & (L <= max_range) & (z_lo <= Dz) & (Dz <= z_hi) & in_grid
    cell = np.where(hit[:, None], hq, 0).astype(np.int64)
    return dict(D=D, t_end=t_end, walked=walked, hit=hit, hit_cell=cell)


def walk(geo, origin32, pts32, p):
    """Step 5 for one scan's rays.  dict(ray (m,), cell (m, 2): every (ray, cell) visit in step order, in the grid or not;
    walked (n,) bool; hit (n,) bool; hit_cell (n, 2))"""
    r = _f(geo["resolution"])
    O2, c0, ok = start_cell(geo, origin32)
    assert ok, "the caller checks the origin's range first"
    R = rays(geo, origin32, pts32, p)
    ids = np.flatnonzero(R["walked"])
    out = dict(ray=np.zeros(0, np.int64), cell=np.zeros((0, 2), np.int64), walked=R["walked"], hit=R["hit"], hit_cell=R["hit_cell"])
    if len(ids) == 0:
        return out
    guard = max_steps(p["max_range"], geo["resolution"])
    D = R["D"][ids][:, :2]
    te = R["t_end"][ids]
    c = np.tile(c0.astype(np.int64), (len(ids), 1))
    s = np.where(D > 0, 1, -1).astype(np.int64)
    Ob = np.tile(O2, (len(ids), 1))
    t = _t_of(c, s, Ob, D, r)
    rays_, cells = [], []
    alive = np.arange(len(ids))
    steps = 0
    while len(alive):
        assert steps < guard, "the step bound of the definition must never bind"
        steps += 1
        rays_.append(ids[alive])                                  # 1. the current cell counts as passed
        cells.append(c[alive].copy())
        ta = t[alive]
        a = np.where(ta[:, 0] <= ta[:, 1], 0, 1)                   # 2. the smaller t_a, ties to x
        go = ta[np.arange(len(alive)), a] <= te[alive]            # 3.
        alive, a = alive[go], a[go]
        c[alive, a] += s[alive, a]                                # 4. recomputed from the new cell
        t[alive, a] = _t_of(c[alive, a], s[alive, a], Ob[alive, a], D[alive, a], r)
    out.update(ray=np.concatenate(rays_), cell=np.concatenate(cells))
    return out


def scan_bits(geo, pose, xyz, p):
    """One scan at its pose: dict(hit, passed: (height, width) bool; walked, marked, visited: the scan's share of the stats)"""
    W, H = int(geo["width"]), int(geo["height"])
    x, _ = A.transform(pose, xyz, np.zeros_like(np.asarray(xyz, np.float32).reshape(-1, 3)))
    w = walk(geo, origin_of(pose), x, p)
    hit, passed = np.zeros((H, W), bool), np.zeros((H, W), bool)
    hc = w["hit_cell"][w["hit"]]
    hit[hc[:, 1], hc[:, 0]] = True
    c = w["cell"]
    inside = (c[:, 0] >= 0) & (c[:, 0] < W) & (c[:, 1] >= 0) & (c[:, 1] < H) if len(c) else np.zeros(0, bool)
    passed[c[inside, 1], c[inside, 0]] = True
    return dict(hit=hit, passed=passed, rays=len(x), walked=int(w["walked"].sum()), marked=int(w["hit"].sum()), visited=len(w["ray"]))


def integrate(geo, scans, ids, poses, p, free=None, seen=None):
    """Steps 1 to 6.  scans: list of xyz (or of (xyz, nrm): normals are ignored) in the sensor frame.  dict(error: the
    LOM_ERR_RANGE verdict; free, seen (height, width) uint32, accumulated onto the ones given; stats as lom_occupancy_stats)"""
    W, H = int(geo["width"]), int(geo["height"])
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    free = np.zeros((H, W), np.int64) if free is None else np.asarray(free).astype(np.int64)
    seen = np.zeros((H, W), np.int64) if seen is None else np.asarray(seen).astype(np.int64)
    out = dict(error=False, free=free.astype(np.uint32), seen=seen.astype(np.uint32), stats=None)
    for k in range(len(ids)):  # the verdict comes before anything changes (an origin counts even for an empty scan)
        if not start_cell(geo, origin_of(poses[k]))[2]:
            out["error"] = True
            return out
    st = dict(scans=len(ids), rays_walked=0, rays_skipped=0, endpoints_marked=0, cells_visited=0)
    for k, i in enumerate(ids):
        xyz = scans[int(i)]
        if isinstance(xyz, tuple):
            xyz = xyz[0]
        b = scan_bits(geo, poses[k], xyz, p)
        seen += b["hit"]
        free += b["passed"] & ~b["hit"]
        st["rays_walked"] += b["walked"]
        st["rays_skipped"] += b["rays"] - b["walked"]
        st["endpoints_marked"] += b["marked"]
        st["cells_visited"] += b["visited"]
    out.update(free=free.astype(np.uint32), seen=seen.astype(np.uint32), stats=st)
    return out


def classify(free, seen, r):
    """step 7: (int8 grid, summary as lom_occupancy_summary)"""
    f, s = np.asarray(free).astype(np.uint64), np.asarray(seen).astype(np.uint64)
    is_free = (f >= int(r["min_free_scans"])) & (f >= np.uint64(int(r["free_per_seen"])) * s)
    is_occ = ~is_free & (s >= int(r["min_seen_scans"]))
    out = np.where(is_free, FREE, np.where(is_occ, OCCUPIED, UNKNOWN)).astype(np.int8)
    return out, dict(cells_free=int(is_free.sum()), cells_occupied=int(is_occ.sum()),
                     cells_unknown=int((~is_free & ~is_occ).sum()))
