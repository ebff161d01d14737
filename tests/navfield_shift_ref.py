"""The shift with a re-solve of the navigation field restated (include/lidar_odometry_amd.h, "navigation field", "Shift and
re-solve"), on top of tests/navfield_ref.py, tests/navfield_resolve_ref.py and tests/grid_shift_ref.py: the moved state, the
merged plane, the three goal counts, cells_changed, cells_raised and the solve that the device must equal byte for byte."""
import numpy as np

from tests import grid_shift_ref as GS
from tests import navfield_ref as N
from tests import navfield_resolve_ref as RR

U = N.UNREACHED


def moved_state(P_old, kept, dx, dy):
    """(P, plane, mask): cell (ix, iy) takes P and the kept byte of cell (ix + dx, iy + dy) where that lies in the grid -- mask
    True, the kept box -- and has entered elsewhere: P unreached, no kept byte (0 here, never read)"""
    P_old, kept = np.asarray(P_old, np.uint32), np.asarray(kept, np.int8)
    h, w = kept.shape
    return GS.shift_array(P_old, dx, dy, U), GS.shift_array(kept, dx, dy, 0), GS.kept_mask(w, h, dx, dy)


def merged_plane(moved, mask, new, window):
    """(merged plane, taken): entered cells and kept cells of the clipped window take the new plane's byte (taken True);
    every other kept cell keeps its own and is not read from the new plane"""
    h, w = moved.shape
    taken = ~mask
    r = RR.clip(w, h, window)
    if r is not None:
        xa, ya, xb, yb = r
        taken[ya:yb, xa:xb] = True
    return np.where(taken, np.asarray(new, np.int8), moved), taken


def goals_left(P_old, dx, dy):
    """the goals (P == 0) whose cell no destination takes"""
    P_old = np.asarray(P_old)
    h, w = P_old.shape
    return int(((P_old == 0) & ~GS.kept_mask(w, h, -dx, -dy)).sum())


def given_plane(new, taken, rng):
    """what a caller may hand over: the new plane where it is read, garbage elsewhere"""
    garbage = rng.integers(-128, 128, new.shape).astype(np.int8)
    return np.where(taken, new, garbage)


def incremental(P_moved, merged, p):
    """the device's way on the reference: drop the impassable cells, raise the least set, relax; (P uint32, cells raised)"""
    c = N.costs_of(merged, p)
    P = RR.as_rows(P_moved)
    RR.drop_impassable(P, c)
    rose = RR.least_raised_set(P, c)
    RR.relax(P, c)
    return RR.to_array(P), len(rose)


def shift_resolve(geo, kept, new, window, p, P_old, dx, dy):
    """What lom_navfield_shift_resolve* must leave.  dict(status; and for OK: geo: the shifted geometry; plane: the merged
    plane; P, summary, costs: navfield_ref.solve of it in the new geometry for the goals of the moved state; cells_changed,
    cells_raised: what lom_navfield_resolve_stats gives (the latter under the default form); cells_kept, cells_entered,
    goals_left: what lom_navfield_shift_stats gives; taken: the cells read from the new plane)."""
    status, g2 = GS.shift_geometry(geo, dx, dy)
    if status != GS.OK:
        return dict(status=status)
    P_moved, moved, mask = moved_state(P_old, kept, dx, dy)
    merged, taken = merged_plane(moved, mask, new, window)
    g2 = dict(g2, origin_x=float(g2["origin_x"]), origin_y=float(g2["origin_y"]))
    full = N.solve(g2, merged, p, RR.derived_goals(P_moved))
    c = full["costs"]
    P = RR.as_rows(P_moved)
    RR.drop_impassable(P, c)
    return dict(status=GS.OK, geo=g2, plane=merged, P=full["P"], summary=full["summary"], costs=c, taken=taken,
                cells_changed=int((mask & taken & (merged != moved)).sum()), cells_raised=len(RR.least_raised_set(P, c)),
                cells_kept=int(mask.sum()), cells_entered=int((~mask).sum()), goals_left=goals_left(P_old, dx, dy), moved_P=P_moved)


def cut(world, ox, oy, w, h, fill=100):
    """the window of w x h cells of a world plane whose cell (0, 0) is the world's (ox, oy); `fill` outside the world"""
    return GS.shift_array(np.pad(world, ((0, max(0, h - world.shape[0])), (0, max(0, w - world.shape[1]))), constant_values=fill),
                          ox, oy, fill)[:h, :w]
