"""Reference of ray carving (include/lidar_odometry_amd.h, "ray carving"): the definition restated in numpy f64 from the
header's text, vectorised over rays with a loop over steps, and the geometry it is checked against.

Stored set and creation order: the oracle map (oracle/oracle.py) -- its full export lists the voxels in creation order,
the points of one voxel together; a voxel is named by the map's own index rule (f32 division, truncation toward zero).
The oracle has no erase by voxel: a carved map is the export without the erased voxels' points (an erase in place and a
compaction export the same), and `regrow` puts exactly those points into a fresh oracle map, where a later insert then
does what the reference's insert does.
"""
import math

import numpy as np

LIMIT = 1 << 20  # |index| stays below (lom_internal.hpp, voxel_index)


def params(margin, min_range, max_range, min_crossings):
    return dict(margin=margin, min_range=min_range, max_range=max_range, min_crossings=min_crossings)


def map_index(xyz32, voxel_size):
    """(index (n, 3) int64, ok (n,)): f32 x / voxel_size, truncated toward zero; ok = finite and |quotient| < 2^20."""
    x = np.asarray(xyz32, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        f = x / np.float32(voxel_size)
    assert f.dtype == np.float32
    ok = np.all((f > -LIMIT) & (f < LIMIT), axis=1)  # (NaN compares false)
    return np.trunc(np.where(ok[:, None], f, 0)).astype(np.int64), ok


def pack(idx):
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    return ((idx[:, 0] + LIMIT) << 42) | ((idx[:, 1] + LIMIT) << 21) | (idx[:, 2] + LIMIT)


def _plane(c, s):
    """next plane index of cell c in direction s: cell 0 spans (-V, V), there is no plane at 0"""
    return np.where(s > 0, np.where(c >= 0, c + 1, c), np.where(c <= 0, c - 1, c))


def _t_of(c, s, O, D, V):
    with np.errstate(all="ignore"):
        t = (_plane(c, s).astype(np.float64) * V - O) / D
    return np.where(D != 0, t, np.inf)


def t_end_of(origin, pts, p):
    """(t_end, walked, L) per ray, f64 from the f32 inputs"""
    O = np.asarray(origin, np.float32).astype(np.float64).reshape(3)
    P = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    D = P - O
    with np.errstate(all="ignore"):
        L = np.sqrt(D[:, 0] * D[:, 0] + (D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2]))
        long_enough = L >= float(np.float32(p["min_range"]))
        t_end = (np.minimum(L, float(np.float32(p["max_range"]))) - float(np.float32(p["margin"]))) / L
    walked = long_enough & (t_end > 0)
    return t_end, walked, L


def walk(origin, pts, voxel_size, p):
    """dict(ray (m,), cell (m, 3): every (ray, cell) visit in step order; walked (n,) bool; error bool; steps)"""
    o32 = np.asarray(origin, np.float32).reshape(3)
    p32 = np.asarray(pts, np.float32).reshape(-1, 3)
    n = len(p32)
    V = float(np.float32(voxel_size))
    _, ok_o = map_index(o32[None], voxel_size)
    _, ok_p = map_index(p32, voxel_size)
    error = (not ok_o.all()) or (not ok_p.all())
    out = dict(ray=np.zeros(0, np.int64), cell=np.zeros((0, 3), np.int64), walked=np.zeros(n, bool), error=bool(error),
               steps=0)
    if error or n == 0:
        return out
    O = o32.astype(np.float64)
    D = p32.astype(np.float64) - O
    t_end, walked, _ = t_end_of(o32, p32, p)
    out["walked"] = walked
    ids = np.flatnonzero(walked)
    if len(ids) == 0:
        return out
    D, t_end = D[ids], t_end[ids]
    c = np.broadcast_to(np.trunc(O / V).astype(np.int64), D.shape).copy()
    s = np.where(D > 0, 1, -1).astype(np.int64)
    Ob = np.broadcast_to(O, D.shape)
    t = _t_of(c, s, Ob, D, V)
    guard = 3 * (math.ceil(float(np.float32(p["max_range"])) / V) + 2)
    rays, cells = [], []
    alive = np.arange(len(ids))
    steps = 0
    while len(alive):
        assert steps < guard, "the step bound of the definition must never bind"
        steps += 1
        rays.append(ids[alive])
        cells.append(c[alive].copy())
        ta = t[alive]
        ax = np.where((ta[:, 0] <= ta[:, 1]) & (ta[:, 0] <= ta[:, 2]), 0, np.where(ta[:, 1] <= ta[:, 2], 1, 2))
        tmin = ta[np.arange(len(alive)), ax]
        go = tmin <= t_end[alive]
        alive, ax = alive[go], ax[go]
        c[alive, ax] += s[alive, ax]
        if np.any(np.abs(c[alive, ax]) >= LIMIT):
            out["error"] = True
            return out
        t[alive, ax] = _t_of(c[alive, ax], s[alive, ax], Ob[alive, ax], D[alive, ax], V)
    out.update(ray=np.concatenate(rays), cell=np.concatenate(cells), steps=steps)
    return out


def voxels_of_export(xyz32, voxel_size):
    """(keys of the live voxels in export order, voxel ordinal of every exported point)"""
    idx, ok = map_index(xyz32, voxel_size)
    assert ok.all()
    k = pack(idx)
    if len(k) == 0:
        return k, np.zeros(0, np.int64)
    first = np.r_[True, k[1:] != k[:-1]]
    keys = k[first]
    assert len(np.unique(keys)) == len(keys), "a voxel's points are exported together"
    return keys, np.cumsum(first) - 1


def carve(export_xyz, voxel_size, origin, pts, p):
    """The definition against the exported map.  dict(error; cross, hit, erase per live voxel in export order;
    point_keep per exported point; stats as lom_carve_stats)."""
    keys, vox_of_pt = voxels_of_export(export_xyz, voxel_size)
    nv = len(keys)
    w = walk(origin, pts, voxel_size, p)
    out = dict(error=w["error"], cross=np.zeros(nv, np.uint32), hit=np.zeros(nv, np.uint8), erase=np.zeros(nv, bool),
               point_keep=np.ones(len(vox_of_pt), bool), stats=None)
    if w["error"]:
        return out
    order = np.argsort(keys)
    skeys = keys[order]

    def lookup(k):  # voxel ordinal or -1
        if nv == 0:
            return np.full(len(k), -1, np.int64)
        pos = np.minimum(np.searchsorted(skeys, k), nv - 1)
        return np.where(skeys[pos] == k, order[pos], -1)

    p32 = np.asarray(pts, np.float32).reshape(-1, 3)
    idx, _ = map_index(p32, voxel_size)
    h = lookup(pack(idx))
    hit = np.zeros(nv, bool)
    hit[h[h >= 0]] = True
    v = lookup(pack(w["cell"]))
    pair = np.stack([w["ray"], w["cell"][:, 0], w["cell"][:, 1], w["cell"][:, 2]], 1)
    assert len(np.unique(pair, axis=0)) == len(pair), "a ray visits a cell at most once"
    cross = np.bincount(v[v >= 0], minlength=nv).astype(np.uint32)
    mc = int(p["min_crossings"])
    erase = (cross >= mc) & ~hit
    n = len(p32)
    n_walked = int(w["walked"].sum())
    out.update(cross=cross, hit=hit.astype(np.uint8), erase=erase, point_keep=~erase[vox_of_pt] if nv else out["point_keep"],
               stats=dict(rays_walked=n_walked, rays_skipped=n - n_walked, cells_visited=len(w["ray"]),
                          voxels_crossed=int((cross > 0).sum()), voxels_protected=int(((cross >= mc) & hit).sum()),
                          voxels_erased=int(erase.sum())))
    return out


def regrow(O, voxel_size, max_points, xyz, nrm):
    """A fresh oracle map that holds exactly these exported points, voxels in this order."""
    g = O.VoxelGrid(float(voxel_size), int(max_points))
    if len(xyz):
        g.addCloud(np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32))
    return g


# ---- geometry: the cells a segment meets, by brute force ----------------------------------------------------------------
def cell_bounds(c, V):
    """[lo, hi] of cell index c along one axis under the truncating index: cell 0 is (-V, V), double width"""
    c = np.asarray(c, np.float64)
    lo = np.where(c > 0, c * V, (c - 1) * V)
    hi = np.where(c < 0, c * V, (c + 1) * V)
    return lo, hi


def cells_met_by_segment(O, D, t_end, V):
    """Set of cells whose box the segment O + t D, t in [0, t_end], intersects: slab test over the bounding block."""
    O, D = np.asarray(O, np.float64), np.asarray(D, np.float64)
    E = O + t_end * D
    lo_c = np.floor(np.minimum(O, E) / V).astype(np.int64) - 2
    hi_c = np.ceil(np.maximum(O, E) / V).astype(np.int64) + 2
    axes = [np.arange(lo_c[a], hi_c[a] + 1) for a in range(3)]
    near = np.full([len(a) for a in axes], 0.0)
    far = np.full([len(a) for a in axes], float(t_end))
    for a in range(3):
        lo, hi = cell_bounds(axes[a], V)
        shape = [1, 1, 1]
        shape[a] = len(axes[a])
        if D[a] == 0:
            inside = (O[a] > lo) & (O[a] < hi)
            t0 = np.where(inside, -np.inf, np.inf)
            t1 = np.where(inside, np.inf, -np.inf)
        else:
            ta, tb = (lo - O[a]) / D[a], (hi - O[a]) / D[a]
            t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)
        near = np.maximum(near, t0.reshape(shape))
        far = np.minimum(far, t1.reshape(shape))
    ix, iy, iz = np.nonzero(near <= far)
    return set(zip(axes[0][ix].tolist(), axes[1][iy].tolist(), axes[2][iz].tolist()))
