"""Steps 8 and 9 of the navigation field restated on Python integers (include/lidar_odometry_amd.h, "navigation field"), on
top of tests/navfield_ref.py: the line-of-sight rule, the greedy choice of waypoints along a step-6 route, and -- as a
check of the rule itself -- an independent line of sight that clips the segment between the two cell centres against
every cell on exact fractions.  Everything is an integer or a Fraction, so every comparison with the device is exact."""
from fractions import Fraction

import numpy as np

from tests import navfield_ref as N


def clear(c, max_cell_cost):
    return c != 0 and (max_cell_cost == 0 or c <= max_cell_cost)


def visible(c, w, h, a, b, max_cell_cost=0):
    """step 8: c as navfield_ref.costs_of gives it (rows of Python integers); a, b: (x, y)"""
    (x0, y0), (x1, y1) = a, b
    if not (0 <= x0 < w and 0 <= y0 < h and 0 <= x1 < w and 0 <= y1 < h):
        return False
    dx, dy = x1 - x0, y1 - y0
    ax, ay, sx, sy = abs(dx), abs(dy), (1 if dx >= 0 else -1), (1 if dy >= 0 else -1)
    i = j = 0
    x, y = x0, y0
    while (i, j) != (ax, ay):
        lhs, rhs = (2 * i + 1) * ay, (2 * j + 1) * ax
        if lhs < rhs:
            x, i = x + sx, i + 1
        elif lhs > rhs:
            y, j = y + sy, j + 1
        else:
            if not (clear(c[y][x + sx], max_cell_cost) and clear(c[y + sy][x], max_cell_cost)):
                return False
            x, y, i, j = x + sx, y + sy, i + 1, j + 1
        if not clear(c[y][x], max_cell_cost):
            return False
    return True


def visible_by_fractions(c, w, h, a, b, max_cell_cost=0):
    """The same question without the walk.  The segment joins the centres of a and b.  Every cell other than a whose open
    interior meets the open segment is clear, and at every lattice point strictly inside the segment all four cells round
    it, a excepted, are clear: the two the segment runs through and the two beside it."""
    (x0, y0), (x1, y1) = a, b
    if not (0 <= x0 < w and 0 <= y0 < h and 0 <= x1 < w and 0 <= y1 < h):
        return False
    if a == b:
        return True
    half = Fraction(1, 2)
    px, py, dx, dy = x0 + half, y0 + half, x1 - x0, y1 - y0

    def span(p, d, lo):
        """the open interval of t with lo < p + t d < lo + 1, or None"""
        if d == 0:
            return (Fraction(-1), Fraction(2)) if lo < p < lo + 1 else None
        t0, t1 = (lo - p) / d, (lo + 1 - p) / d
        return (min(t0, t1), max(t0, t1))

    for y in range(min(y0, y1), max(y0, y1) + 1):
        for x in range(min(x0, x1), max(x0, x1) + 1):
            if (x, y) == a:
                continue
            sx_, sy_ = span(px, dx, x), span(py, dy, y)
            if sx_ is None or sy_ is None:
                continue
            lo, hi = max(sx_[0], sy_[0], Fraction(0)), min(sx_[1], sy_[1], Fraction(1))
            if lo < hi and not clear(c[y][x], max_cell_cost):
                return False
    if dx and dy:
        for X in range(min(x0, x1) + 1, max(x0, x1) + 1):           # the lattice lines between the centres
            t = (X - px) / dx
            Y = py + t * dy
            if 0 < t < 1 and Y.denominator == 1:
                for cx, cy in ((X - 1, int(Y) - 1), (X, int(Y) - 1), (X - 1, int(Y)), (X, int(Y))):
                    if (cx, cy) != a and not clear(c[cy][cx], max_cell_cost):
                        return False
    return True


def shortcut(route, lookahead, see):
    """step 9 for one route (a list of cells): the waypoints; see(a, b) -> bool"""
    if not route:
        return []
    out, a, n = [route[0]], 0, len(route)
    while a < n - 1:
        nxt = a + 1
        for j in range(min(a + lookahead, n - 1), a + 1, -1):
            if see(route[a], route[j]):
                nxt = j
                break
        a = nxt
        out.append(route[a])
    return out


def tested_per_anchor(route, lookahead, see):
    """(anchors, candidates tested one after another from the farthest) of a route: what the serial form walks"""
    anchors = tested = a = 0
    n = len(route)
    while a < n - 1:
        nxt = a + 1
        for j in range(min(a + lookahead, n - 1), a + 1, -1):
            tested += 1
            if see(route[a], route[j]):
                nxt = j
                break
        a, anchors = nxt, anchors + 1
    return anchors, tested


def waypoints(geo, c, P, starts, max_cell_cost, lookahead, route_cap, wp_cap, metres=False):
    """(cells uint16 (K, wp_cap, 2), counts uint32 (K,), lengths uint32 (K,)) as lom_navfield_waypoints writes them"""
    w, h = geo["width"], geo["height"]
    cells_in = N.cells_of(geo, starts, metres)
    cells = np.zeros((len(cells_in), wp_cap, 2), np.uint16)
    counts, lengths = np.zeros(len(cells_in), np.uint32), np.zeros(len(cells_in), np.uint32)
    for k, s in enumerate(cells_in):
        route = N.path(geo, c, P, s)
        lengths[k] = len(route)
        wp = shortcut(route[:route_cap], lookahead, lambda a, b: visible(c, w, h, a, b, max_cell_cost))
        counts[k] = len(wp)
        if wp and wp_cap:
            head = np.array(wp[:wp_cap], np.uint16)
            cells[k, :len(head)] = head
    return cells, counts, lengths


def visible_many(c, w, h, pairs, max_cell_cost=0):
    """uint8 per (x0, y0, x1, y1) as lom_navfield_visible writes them"""
    return np.array([visible(c, w, h, (int(q[0]), int(q[1])), (int(q[2]), int(q[3])), max_cell_cost)
                     for q in np.asarray(pairs).reshape(-1, 4)], np.uint8)


def polyline_cells(cells):
    """the Euclidean length of a polyline through cells, in cells"""
    p = np.asarray(cells, np.float64).reshape(-1, 2)
    return float(np.sqrt((np.diff(p, axis=0) ** 2).sum(axis=1)).sum())
