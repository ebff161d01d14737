"""The navigation field restated on Python integers (include/lidar_odometry_amd.h, "navigation field"): the cell-cost
table, the allowed steps, goals, the field by a heap Dijkstra from the goals, the summary with range_exceeded, the path
rule and the query.  tests/test_navfield_host.py checks the field against scipy's Dijkstra on the same graph and against a
brute-force Bellman-Ford.  Everything is an integer, so every comparison with the device is exact."""
import heapq

import numpy as np

UNREACHED, MAX = 0xFFFFFFFF, 0xFFFFFFFE
UNKNOWN_PASSABLE = 1
MAX_CELL_COST = (1 << 24) - 1
SUMMARY_KEYS = ("cells_blocked", "cells_reached", "cells_unreached", "cells_invalid", "goals_used", "goals_rejected",
                "range_exceeded", "max_potential")
# the fixed order of step 6: E, N, W, S, NE, NW, SW, SE (+x is E, +y is N), as (dx, dy, length)
STEPS = ((1, 0, 5), (0, 1, 5), (-1, 0, 5), (0, -1, 5), (1, 1, 7), (-1, 1, 7), (-1, -1, 7), (1, -1, 7))


def geometry(resolution, origin_x, origin_y, width, height):
    return dict(resolution=np.float32(resolution), origin_x=np.float32(origin_x), origin_y=np.float32(origin_y),
                width=int(width), height=int(height))


def params(neutral, factor, unknown_cost, max_passable, flags=0):
    return dict(neutral=int(neutral), factor=int(factor), unknown_cost=int(unknown_cost), max_passable=int(max_passable),
                flags=int(flags))


def params_ok(p):
    if p["neutral"] < 1 or p["neutral"] >= 1 << 32 or not 0 <= p["factor"] < 1 << 32 or not 0 <= p["max_passable"] <= 98:
        return False
    if p["flags"] & ~UNKNOWN_PASSABLE or p["neutral"] + 98 * p["factor"] > MAX_CELL_COST:
        return False
    return not (p["flags"] & UNKNOWN_PASSABLE) or 1 <= p["unknown_cost"] <= MAX_CELL_COST


def cell_costs(p):
    """step 1: 256 Python integers, indexed by the cost byte read as unsigned; 0 = impassable"""
    t = [0] * 256
    for v in range(p["max_passable"] + 1):
        t[v] = p["neutral"] + p["factor"] * v
    if p["flags"] & UNKNOWN_PASSABLE:
        t[255] = p["unknown_cost"]
    return t


def costs_of(plane, p):
    """c per cell as a list of rows of Python integers"""
    t = cell_costs(p)
    return [[t[int(b)] for b in row] for row in np.asarray(plane, np.int8).view(np.uint8)]


def allowed(c, w, h, x, y, dx, dy):
    """whether the step between the passable cell (x, y) and (x + dx, y + dy) is allowed (the rule is symmetric)"""
    bx, by = x + dx, y + dy
    if not (0 <= bx < w and 0 <= by < h) or not c[by][bx]:
        return False
    return not (dx and dy) or bool(c[y][bx] and c[by][x])


def cell_of_metres(geo, x, y):
    """the floor rule: (ix, iy), or None outside the grid or for a value that is no number"""
    r = np.float64(geo["resolution"])
    with np.errstate(invalid="ignore", over="ignore"):
        qx = np.floor((np.float64(np.float32(x)) - np.float64(geo["origin_x"])) / r)
        qy = np.floor((np.float64(np.float32(y)) - np.float64(geo["origin_y"])) / r)
    if 0 <= qx < geo["width"] and 0 <= qy < geo["height"]:
        return int(qx), int(qy)
    return None


def cells_of(geo, points, metres):
    """a list of (ix, iy) or None per point"""
    out = []
    for a, b in np.asarray(points).reshape(-1, 2):
        if metres:
            out.append(cell_of_metres(geo, a, b))
        else:
            out.append((int(a), int(b)) if 0 <= a < geo["width"] and 0 <= b < geo["height"] else None)
    return out


def solve(geo, plane, p, goals, metres=False):
    """dict(P uint32 (h, w), summary, error).  A refused solve has error=True and a summary of zeros."""
    w, h = geo["width"], geo["height"]
    zero = dict.fromkeys(SUMMARY_KEYS, 0)
    if not params_ok(p):
        return dict(P=None, summary=zero, error=True)
    plane = np.asarray(plane, np.int8)
    assert plane.shape == (h, w)
    c = costs_of(plane, p)
    P = [[UNREACHED] * w for _ in range(h)]
    heap, used, rejected = [], set(), 0
    for cell in cells_of(geo, goals, metres):
        if cell is None or not c[cell[1]][cell[0]]:
            rejected += 1
        elif cell not in used:
            used.add(cell)
            P[cell[1]][cell[0]] = 0
            heap.append((0, cell[0], cell[1]))
    heapq.heapify(heap)
    while heap:
        pb, bx, by = heapq.heappop(heap)
        if pb != P[by][bx]:
            continue
        for dx, dy, ln in STEPS:                                   # the step a -> b pays for a, the cell it leaves
            if allowed(c, w, h, bx, by, dx, dy):
                ax, ay = bx + dx, by + dy
                cand = pb + ln * c[ay][ax]
                if cand <= MAX and cand < P[ay][ax]:
                    P[ay][ax] = cand
                    heapq.heappush(heap, (cand, ax, ay))
    exceeded = 0
    for by in range(h):
        for bx in range(w):
            if P[by][bx] != UNREACHED and P[by][bx] > MAX - 7 * MAX_CELL_COST:
                for dx, dy, ln in STEPS:
                    if allowed(c, w, h, bx, by, dx, dy) and P[by][bx] + ln * c[by + dy][bx + dx] > MAX:
                        exceeded = 1
    Pa = np.array(P, dtype=np.uint64).astype(np.uint32).reshape(h, w)
    passable = np.array(c, dtype=np.uint64).reshape(h, w) != 0
    reached = Pa != UNREACHED
    pv = plane.astype(int)
    summary = dict(cells_blocked=int((~passable).sum()), cells_reached=int(reached.sum()),
                   cells_unreached=int((passable & ~reached).sum()), cells_invalid=int(((pv < -1) | (pv > 100)).sum()),
                   goals_used=len(used), goals_rejected=rejected, range_exceeded=exceeded,
                   max_potential=int(Pa[reached].max()) if reached.any() else 0)
    return dict(P=Pa, summary=summary, error=False, costs=c)


def path(geo, c, P, start):
    """step 6 from one start cell ((ix, iy) or None): the list of cells, [] where none is walked"""
    w, h = geo["width"], geo["height"]
    if start is None or int(P[start[1], start[0]]) == UNREACHED:
        return []
    x, y = start
    out = [(x, y)]
    while int(P[y, x]) > 0:
        for dx, dy, ln in STEPS:
            if allowed(c, w, h, x, y, dx, dy) and int(P[y + dy, x + dx]) != UNREACHED and \
                    int(P[y + dy, x + dx]) + ln * c[y][x] == int(P[y, x]):
                x, y = x + dx, y + dy
                break
        else:
            raise AssertionError("no step down the field at %r" % ((x, y),))
        out.append((x, y))
    return out


def paths(geo, c, P, starts, cap, metres=False):
    """(cells uint16 (K, cap, 2), lengths uint32 (K,)) as lom_navfield_paths writes them: the rest of a row is 0"""
    cells_in = cells_of(geo, starts, metres)
    cells, lengths = np.zeros((len(cells_in), cap, 2), np.uint16), np.zeros(len(cells_in), np.uint32)
    for k, s in enumerate(cells_in):
        route = path(geo, c, P, s)
        lengths[k] = len(route)
        if route and cap:
            head = np.array(route[:cap], np.uint16)
            cells[k, :len(head)] = head
    return cells, lengths


def path_weight(c, route):
    """the sum of len * c[a] over the steps of a route, and whether every step is one cell far"""
    total = 0
    for (ax, ay), (bx, by) in zip(route, route[1:]):
        dx, dy = bx - ax, by - ay
        assert max(abs(dx), abs(dy)) == 1
        total += (7 if dx and dy else 5) * c[ay][ax]
    return total


def query(geo, P, xy):
    """uint32 per point: the cell's P, UNREACHED outside the grid"""
    out = np.full(len(np.asarray(xy).reshape(-1, 2)), UNREACHED, np.uint32)
    for i, cell in enumerate(cells_of(geo, xy, True)):
        if cell is not None:
            out[i] = P[cell[1], cell[0]]
    return out
