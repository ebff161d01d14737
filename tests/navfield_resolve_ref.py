"""The re-solve of the navigation field restated on Python integers (include/lidar_odometry_amd.h, "navigation field",
"Re-solve"), on top of tests/navfield_ref.py: the merged plane, the derived goals, the least raised set by the safety
rule, the threshold set, and the relaxation of what is left.  resolve() gives what the device must leave: the full solve of
the merged plane for the derived goals, with the counts of the diff and of the raise phase."""
import heapq

import numpy as np

from tests import navfield_ref as N

U = N.UNREACHED


def clip(w, h, window):
    """the window (x0, y0, width, height) clipped to the grid as (xa, ya, xb, yb); None: the whole grid; empty: None"""
    if window is None:
        return 0, 0, w, h
    x0, y0, ww, hh = (int(v) for v in window)
    xa, ya, xb, yb = max(x0, 0), max(y0, 0), min(x0 + ww, w), min(y0 + hh, h)
    return (xa, ya, xb, yb) if xa < xb and ya < yb else None


def merged_plane(kept, new, window):
    """the kept plane with the cells of the clipped window replaced by the new plane's; cells outside it are not read"""
    kept = np.asarray(kept, np.int8)
    h, w = kept.shape
    out, r = kept.copy(), clip(w, h, window)
    if r is not None:
        xa, ya, xb, yb = r
        out[ya:yb, xa:xb] = np.asarray(new, np.int8)[ya:yb, xa:xb]
    return out


def derived_goals(P):
    """the cells with P == 0, as (ix, iy) rows"""
    return np.argwhere(np.asarray(P) == 0)[:, ::-1].astype(np.int32).reshape(-1, 2)


def as_rows(P):
    return [[int(v) for v in row] for row in P]


def drop_impassable(P, c):
    """the diff's part: a reached cell that is impassable reads unreached; returns how many"""
    n = 0
    for y, row in enumerate(P):
        for x, p in enumerate(row):
            if p != U and not c[y][x]:
                row[x] = U
                n += 1
    return n


def least_raised_set(P, c):
    """The raise phase on rows of Python integers P (impassable cells unreached already), in place: in increasing order of
    P, a reached cell a with P[a] > 0 stays iff some allowed step a -> b has P[b] reached and P[b] + len * c[a] <= P[a].
    Supporters have strictly lower P, so when a cell's turn comes its supporters are final.  Returns the set of cells that
    rose."""
    h, w = len(P), len(P[0])
    rose = set()
    for p, x, y in sorted((P[y][x], x, y) for y in range(h) for x in range(w) if P[y][x] != U and P[y][x] > 0):
        for dx, dy, ln in N.STEPS:
            if N.allowed(c, w, h, x, y, dx, dy) and P[y + dy][x + dx] != U and P[y + dy][x + dx] + ln * c[y][x] <= p:
                break
        else:
            P[y][x] = U
            rose.add((x, y))
    return rose


def threshold_set(P, changed):
    """The threshold form on rows P as they were before the diff touched them, in place (impassable cells are the caller's to
    drop afterwards): pmin is the least positive P among the changed cells and their eight neighbours; every reached cell
    with P > 0 and P >= pmin reads unreached.  Returns the set of cells that rose."""
    h, w = len(P), len(P[0])
    ring = {(x + dx, y + dy) for x, y in changed for dx in (-1, 0, 1) for dy in (-1, 0, 1) if 0 <= x + dx < w and 0 <= y + dy < h}
    vals = [P[y][x] for x, y in ring if P[y][x] != U and P[y][x] > 0]
    rose = set()
    if vals:
        pmin = min(vals)
        for y in range(h):
            for x in range(w):
                if P[y][x] != U and P[y][x] >= pmin and P[y][x] > 0:
                    P[y][x] = U
                    rose.add((x, y))
    return rose


def relax(P, c):
    """the relaxation from upper bounds, in place, to its fixed point: a heap over every reached cell"""
    h, w = len(P), len(P[0])
    heap = [(P[y][x], x, y) for y in range(h) for x in range(w) if P[y][x] != U]
    heapq.heapify(heap)
    while heap:
        pb, bx, by = heapq.heappop(heap)
        if pb != P[by][bx]:
            continue
        for dx, dy, ln in N.STEPS:
            if N.allowed(c, w, h, bx, by, dx, dy):
                ax, ay = bx + dx, by + dy
                cand = pb + ln * c[ay][ax]
                if cand <= N.MAX and cand < P[ay][ax]:
                    P[ay][ax] = cand
                    heapq.heappush(heap, (cand, ax, ay))


def to_array(P):
    return np.array(P, dtype=np.uint64).astype(np.uint32)


def changed_cells(kept, merged):
    """the cells whose byte differs, as a set of (x, y)"""
    return {(int(x), int(y)) for y, x in np.argwhere(np.asarray(kept, np.int8) != np.asarray(merged, np.int8))}


def raise_then_relax(P_old, kept, merged, p, form):
    """The incremental forms on the reference: (P uint32, cells raised).  form 0: the least set; form 1: the threshold."""
    c = N.costs_of(merged, p)
    P = as_rows(P_old)
    if form == 0:
        drop_impassable(P, c)
        rose = least_raised_set(P, c)
    else:
        rose = threshold_set(P, changed_cells(kept, merged))
        rose = {(x, y) for x, y in rose if c[y][x]}       # (what the diff dropped is not the reset's)
        drop_impassable(P, c)
    relax(P, c)
    return to_array(P), len(rose)


def resolve(geo, kept, new, window, p, P_old, with_threshold=False):
    """What a re-solve must leave: dict(plane: the merged plane, P, summary, costs: navfield_ref.solve of it for the derived
    goals; cells_changed; cells_raised: the size of the least raised set; [cells_raised_threshold])."""
    merged = merged_plane(kept, new, window)
    full = N.solve(geo, merged, p, derived_goals(P_old))
    c = full["costs"]
    P = as_rows(P_old)
    drop_impassable(P, c)
    out = dict(plane=merged, P=full["P"], summary=full["summary"], costs=c, cells_changed=len(changed_cells(kept, merged)),
               cells_raised=len(least_raised_set(P, c)))
    if with_threshold:
        out["cells_raised_threshold"] = raise_then_relax(P_old, kept, merged, p, 1)[1]
    return out
