"""Reference of the scan votes (include/lidar_odometry_amd.h, "scan votes"): the definition restated in numpy f64 from the
header's text.  The transform is assemble_ref's, the index rule, the plane rule and the export's voxel order are
carve_ref's; the walk is written again here, with the votes' own t_end, so that with clearance = 0 it can be compared
with carve_ref.walk."""
import math

import numpy as np

from tests import assemble_ref as A
from tests import carve_ref as R

LIMIT = R.LIMIT


def params(margin, min_range, max_range, clearance, min_free_scans, free_per_seen):
    return dict(margin=margin, min_range=min_range, max_range=max_range, clearance=clearance,
                min_free_scans=min_free_scans, free_per_seen=free_per_seen)


def t_end_of(origin, pts, nrm, p):
    """(t_end, walked, L) per ray: step 4 of the header, f64 from the f32 inputs, every operation on its own"""
    O = np.asarray(origin, np.float32).astype(np.float64).reshape(3)
    P = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    N = np.asarray(nrm, np.float32).astype(np.float64).reshape(-1, 3)
    D = P - O
    margin, min_range, max_range, clearance = (float(np.float32(p[k])) for k in ("margin", "min_range", "max_range", "clearance"))
    with np.errstate(all="ignore"):
        L = np.sqrt(D[:, 0] * D[:, 0] + (D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2]))
        c = np.abs(N[:, 0] * D[:, 0] + (N[:, 1] * D[:, 1] + N[:, 2] * D[:, 2])) / L
        reach = np.where(L < max_range, L, max_range) - margin
        plane = L - clearance / c if clearance > 0 else reach
        t_end = np.where(plane < reach, plane, reach) / L
        walked = (L >= min_range) & (t_end > 0)
    return t_end, walked, L


def walk(origin, pts, nrm, voxel_size, p):
    """One scan's rays.  dict(ray (m,), cell (m, 3): every (ray, cell) visit in step order; walked (n,) bool; error)"""
    o32 = np.asarray(origin, np.float32).reshape(3)
    p32 = np.asarray(pts, np.float32).reshape(-1, 3)
    n = len(p32)
    V = float(np.float32(voxel_size))
    error = not (R.map_index(o32[None], voxel_size)[1].all() and R.map_index(p32, voxel_size)[1].all())
    out = dict(ray=np.zeros(0, np.int64), cell=np.zeros((0, 3), np.int64), walked=np.zeros(n, bool), error=bool(error))
    if error or n == 0:
        return out
    O = o32.astype(np.float64)
    t_end, walked, _ = t_end_of(o32, p32, nrm, p)
    out["walked"] = walked
    guard = 3 * (math.ceil(float(np.float32(p["max_range"])) / V) + 2)
    ids = np.flatnonzero(walked)
    if len(ids) == 0:
        return out
    # all walked rays advance together, a step of the loop at a time: row r is ray ids[r]
    D = p32[ids].astype(np.float64) - O
    te = t_end[ids]
    c = np.tile(np.trunc(O / V).astype(np.int64), (len(ids), 1))
    s = np.where(D > 0, 1, -1).astype(np.int64)
    Ob = np.tile(O, (len(ids), 1))
    t = R._t_of(c, s, Ob, D, V)  # ((b_a V) - O_a) / D_a with b_a by the plane rule; +inf where D_a == 0
    rays, cells = [], []
    alive = np.arange(len(ids))
    steps = 0
    while len(alive):
        assert steps < guard, "the step bound of the definition must never bind"
        steps += 1
        rays.append(ids[alive])                                   # 1. the current cell counts as crossed
        cells.append(c[alive].copy())
        ta = t[alive]
        a = np.where((ta[:, 0] <= ta[:, 1]) & (ta[:, 0] <= ta[:, 2]), 0, np.where(ta[:, 1] <= ta[:, 2], 1, 2))  # 2.
        go = ta[np.arange(len(alive)), a] <= te[alive]            # 3.
        alive, a = alive[go], a[go]
        c[alive, a] += s[alive, a]                                # 4.
        if np.any(np.abs(c[alive, a]) >= LIMIT):                  # 5.
            out["error"] = True
            return out
        t[alive, a] = R._t_of(c[alive, a], s[alive, a], Ob[alive, a], D[alive, a], V)
    out.update(ray=np.concatenate(rays), cell=np.concatenate(cells))
    return out


def origin_of(pose):
    """the pose's translation, each component rounded to f32"""
    with np.errstate(all="ignore"):
        return np.asarray(pose, np.float64)[:3].astype(np.float32)


def vote(export_xyz, voxel_size, scans, ids, poses, p):
    """The definition against the exported map.  scans: list of (xyz, nrm) in the sensor frame, as the archive holds them.
    dict(error; free, seen, erase per live voxel in export order; point_keep per exported point; stats as lom_vote_stats)"""
    keys, vox_of_pt = R.voxels_of_export(export_xyz, voxel_size)
    nv = len(keys)
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    out = dict(error=False, free=np.zeros(nv, np.uint32), seen=np.zeros(nv, np.uint32), erase=np.zeros(nv, bool),
               point_keep=np.ones(len(vox_of_pt), bool), stats=None)
    order = np.argsort(keys)
    skeys = keys[order]

    def lookup(k):  # voxel ordinal or -1
        if nv == 0 or len(k) == 0:
            return np.full(len(k), -1, np.int64)
        pos = np.minimum(np.searchsorted(skeys, k), nv - 1)
        return np.where(skeys[pos] == k, order[pos], -1)

    free, seen = np.zeros(nv, np.int64), np.zeros(nv, np.int64)
    rays = walked = visited = 0
    for k, i in enumerate(ids):
        x, n = A.transform(poses[k], *scans[int(i)])
        o = origin_of(poses[k])
        if not R.map_index(o[None], voxel_size)[1].all():  # (an origin counts even for an empty scan)
            out["error"] = True
            return out
        w = walk(o, x, n, voxel_size, p)
        if w["error"]:
            out["error"] = True
            return out
        hit, cross = np.zeros(nv, bool), np.zeros(nv, bool)
        h = lookup(R.pack(R.map_index(x, voxel_size)[0]))
        hit[h[h >= 0]] = True
        v = lookup(R.pack(w["cell"]))
        cross[v[v >= 0]] = True
        seen += hit
        free += cross & ~hit
        rays += len(x)
        walked += int(w["walked"].sum())
        visited += len(w["ray"])
    mf, fps = int(p["min_free_scans"]), int(p["free_per_seen"])
    enough = free >= mf
    ratio = free >= fps * seen
    erase = enough & ratio
    out.update(free=free.astype(np.uint32), seen=seen.astype(np.uint32), erase=erase,
               point_keep=~erase[vox_of_pt] if nv else out["point_keep"],
               stats=dict(scans=len(ids), rays_walked=walked, rays_skipped=rays - walked, cells_visited=visited,
                          voxels_free=int((free > 0).sum()), voxels_protected=int((enough & ~ratio).sum()),
                          voxels_erased=int(erase.sum())))
    return out
