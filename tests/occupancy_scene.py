"""The corridor scene of the occupancy grid: the twelve scans of tests/vote_scene.py (normals ignored), the grid they vote
on, and the masks on cell centres that tests/test_occupancy_host.py judges the reference by.  Used on the reference alone
there and against the device in tests/test_occupancy_gpu.py."""
import functools

import numpy as np

from lidar_odometry_demo_amd import synth
from tests import occupancy_ref as O
from tests import vote_scene as S

RES = 0.25
GEO = O.geometry(resolution=RES, origin_x=-70.0, origin_y=-15.0, width=584, height=120)
PARAMS = O.ray_params(z_lo=-1.5, z_hi=0.6, margin=0.0, min_range=2.0, max_range=60.0)
RULE = O.rule(min_free_scans=3, free_per_seen=2, min_seen_scans=1)
X_LO, X_HI = -20.0, 25.0  # the stretch of the corridor the conditions look at


def centres():
    """(X (height, width), Y (height, width)) of the cell centres"""
    x = GEO["origin_x"] + (np.arange(GEO["width"]) + 0.5) * RES
    y = GEO["origin_y"] + (np.arange(GEO["height"]) + 0.5) * RES
    return np.meshgrid(x, y)


def swept_mask():
    """where the mover has been, a cell in from every side (and where the corridor's scans still look: y < 11)"""
    X, Y = centres()
    sw = S.SWEPT
    return (X > sw[0] + RES) & (X < sw[3] - RES) & (Y > sw[1] + RES) & (Y < min(sw[4], 11.0) - RES)


def corridor_mask():
    """between the walls, two cells in, without the static boxes that stand in the height band, each grown by a cell"""
    X, Y = centres()
    m = (np.abs(Y) < synth.WALL_Y - 2 * RES) & (X > X_LO) & (X < X_HI)
    for b in S.static_boxes():
        if b[2] <= -1.2 and b[5] >= 0.0:
            m &= ~((X > b[0] - RES) & (X < b[3] + RES) & (Y > b[1] - RES) & (Y < b[4] + RES))
    return m


def wall_columns(cls):
    """per wall (-WALL_Y, +WALL_Y): the share of the columns X_LO < x < X_HI with an occupied cell within a cell of it"""
    X, Y = centres()
    cols = (X[0] > X_LO) & (X[0] < X_HI)
    out = []
    for wy in (-synth.WALL_Y, synth.WALL_Y):
        near = np.abs(Y - wy) < RES
        has = ((cls == O.OCCUPIED) & near).any(axis=0)
        out.append(float(has[cols].sum()) / int(cols.sum()))
    return out


@functools.lru_cache(maxsize=None)
def reference(mover):
    """the definition on the scene, computed once: dict(free, seen, stats, cls, summary) -- left unchanged by its users"""
    s = S.scene(mover)
    ref = O.integrate(GEO, s["scans"], s["ids"], s["poses"], PARAMS)
    assert not ref["error"]
    cls, summary = O.classify(ref["free"], ref["seen"], RULE)
    ref.update(cls=cls, summary=summary)
    for k in ("free", "seen", "cls"):
        ref[k].setflags(write=False)
    return ref


def measures(mover):
    """the figures of the conditions, as fractions"""
    ref = reference(mover)
    sw, co = swept_mask(), corridor_mask()
    cls = ref["cls"]
    walls = wall_columns(cls)
    return dict(swept_cells=int(sw.sum()), corridor_cells=int(co.sum()),
                swept_seen=float((ref["seen"][sw] >= 1).mean()), swept_free=float((cls[sw] == O.FREE).mean()),
                corridor_free=float((cls[co] == O.FREE).mean()), corridor_occupied=float((cls[co] == O.OCCUPIED).mean()),
                wall_lo=walls[0], wall_hi=walls[1])
