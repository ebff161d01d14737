"""The pose field restated on Python integers (include/lidar_odometry_amd.h, "pose field"): the headings, the stencils of a
footprint, the layers, the six moves, goals, the field by a heap Dijkstra on the reversed moves, the floor, the summary with
range_exceeded, the path rule and the query.  move() states the move rule for one state; moves_of() states it again for
all states at once (numpy, int64: every value is below 2^33), which is what the Dijkstra runs on -- tests/
test_posefield_host.py checks the two against each other, the field against scipy's Dijkstra over the explicit state graph
and against a brute-force Bellman-Ford.  Everything is an integer, so every comparison with the device is exact."""
import heapq
import math

import numpy as np

from tests import navfield_ref as N

UNREACHED, MAX = N.UNREACHED, N.MAX
SPIN, REVERSE = 1, 2
H, MOVES = 8, 6
MAX_COST = (1 << 24) - 1
# heading h points along E, NE, N, NW, W, SW, S, SE (+x is E, +y is N)
HX = (1, 1, 0, -1, -1, -1, 0, 1)
HY = (0, 1, 1, 1, 0, -1, -1, -1)
LEN = (5, 7, 5, 7, 5, 7, 5, 7)
SUMMARY_KEYS = ("states_blocked", "states_reached", "states_unreached", "cells_reached", "cells_invalid", "goals_used",
                "goals_rejected", "range_exceeded", "max_potential")


def params(nav, turn_cost, spin_cost, reverse_cost, flags=0):
    return dict(nav=dict(nav), turn_cost=int(turn_cost), spin_cost=int(spin_cost), reverse_cost=int(reverse_cost), flags=int(flags))


def as_tuple(p):
    n = p["nav"]
    return ((n["neutral"], n["factor"], n["unknown_cost"], n["max_passable"], n["flags"]), p["turn_cost"], p["spin_cost"],
            p["reverse_cost"], p["flags"])


def params_ok(p):
    if not N.params_ok(p["nav"]) or p["flags"] & ~(SPIN | REVERSE):
        return False
    if not all(0 <= p[k] <= MAX_COST for k in ("turn_cost", "spin_cost", "reverse_cost")):
        return False
    return not (p["flags"] & SPIN) or p["spin_cost"] >= 1


def footprint_ok(fp):
    fp = np.asarray(fp, np.int64).reshape(-1, 2)
    return 1 <= len(fp) <= 1024 and bool((np.abs(fp) <= 16384).all())


def heading_of_angle(a):
    return ((int(a) + 4096) >> 13) & 7


def direction(h):
    """entry 512 h of lom_visibility_table(4096): lround of cos and sin times 32768"""
    def lround(v):
        return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)
    t = 2.0 * math.pi * (512 * h) / 4096.0
    return lround(math.cos(t) * 32768.0), lround(math.sin(t) * 32768.0)


def stencils(footprint):
    """step 2: per heading the distinct cell offsets (dx, dy), sorted by (dy, dx)"""
    out = []
    for h in range(H):
        c, s = direction(h)
        cells = set()
        for fx, fy in np.asarray(footprint, np.int64).reshape(-1, 2).tolist():
            ox, oy = (fx * c - fy * s + 128) >> 8, (fx * s + fy * c + 128) >> 8      # (Python's >> floors, as the arithmetic shift)
            cells.add(((16384 + oy) >> 15, (16384 + ox) >> 15))
        out.append([(dx, dy) for dy, dx in sorted(cells)])
    return out


def shifted(A, dx, dy):
    """B[y, x] = A[y + dy, x + dx], 0 where that is outside the grid"""
    h, w = A.shape
    B = np.zeros_like(A)
    x0, x1, y0, y1 = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
    if x0 < x1 and y0 < y1:
        B[y0:y1, x0:x1] = A[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return B


def layers(plane, p, st):
    """step 3: int64 (8, h, w)"""
    c = np.array(N.cell_costs(p["nav"]), np.int64)[np.asarray(plane, np.int8).view(np.uint8)]
    out = np.zeros((H,) + c.shape, np.int64)
    for h in range(H):
        ok, best = np.ones(c.shape, bool), np.zeros(c.shape, np.int64)
        for dx, dy in st[h]:
            v = shifted(c, dx, dy)
            ok &= v != 0
            best = np.maximum(best, v)
        out[h] = np.where(ok, best, 0)
    return out


def move_target(h, m):
    """(sign, heading) of move m from heading h: the cells it goes along its heading and the heading it ends in"""
    sign = 1 if m <= 2 else -1 if m == 5 else 0
    th = (h + 1) % 8 if m in (1, 3) else (h - 1) % 8 if m in (2, 4) else h
    return sign, th


def move_extra(p, m):
    return (0, p["turn_cost"], p["turn_cost"], p["spin_cost"], p["spin_cost"], p["reverse_cost"])[m]


def move(L, p, x, y, h, m):
    """step 4 for one state whose layer is not 0: (tx, ty, th, weight), or None where move m is not allowed"""
    _, hh, ww = L.shape

    def at(g, ax, ay):
        return int(L[g, ay, ax]) if 0 <= ax < ww and 0 <= ay < hh else 0

    if (m in (3, 4) and not p["flags"] & SPIN) or (m == 5 and not p["flags"] & REVERSE):
        return None
    sign, th = move_target(h, m)
    s = at(h, x, y)
    assert s
    bx, by = x + sign * HX[h], y + sign * HY[h]
    if sign:
        if not at(h, bx, by):
            return None
        if h & 1 and not (at(h, bx, y) and at(h, x, by)):
            return None
    if th != h and not at(th, bx, by):
        return None
    return bx, by, th, (LEN[h] * s if sign else 0) + move_extra(p, m)


def moves_of(L, p):
    """step 4 for all states: a list of (h, m, th, dx, dy, allowed bool (hh, ww), weight int64 (hh, ww)), in the fixed order
    per heading"""
    out = []
    for h in range(H):
        s = L[h]
        for m in range(MOVES):
            if (m in (3, 4) and not p["flags"] & SPIN) or (m == 5 and not p["flags"] & REVERSE):
                continue
            sign, th = move_target(h, m)
            dx, dy = sign * HX[h], sign * HY[h]
            ok = s != 0
            if sign:
                ok = ok & (shifted(s, dx, dy) != 0)
                if h & 1:
                    ok = ok & (shifted(s, dx, 0) != 0) & (shifted(s, 0, dy) != 0)
            if th != h:
                ok = ok & (shifted(L[th], dx, dy) != 0)
            out.append((h, m, th, dx, dy, ok, (LEN[h] * s if sign else np.zeros_like(s)) + move_extra(p, m)))
    return out


def edges_of(L, p):
    """every allowed move as (source state, target state, weight) int64 arrays; a state is h * cells + y * width + x"""
    _, hh, ww = L.shape
    n = hh * ww
    cell = np.arange(n, dtype=np.int64).reshape(hh, ww)
    src, tgt, wgt = [], [], []
    for h, m, th, dx, dy, ok, weight in moves_of(L, p):
        src.append(h * n + cell[ok])
        tgt.append(th * n + cell[ok] + dy * ww + dx)
        wgt.append(weight[ok])
    if not src:
        z = np.zeros(0, np.int64)
        return z, z, z
    return np.concatenate(src), np.concatenate(tgt), np.concatenate(wgt)


def goal_states(L, goals):
    """step 5: (the distinct goal states in the order they are first named, goals_rejected)"""
    _, hh, ww = L.shape
    n = hh * ww
    used, rejected = {}, 0
    for x, y, g in np.asarray(goals, np.int64).reshape(-1, 3).tolist():
        named = []
        if 0 <= x < ww and 0 <= y < hh and -1 <= g <= 7:
            named = [h for h in range(H) if (g < 0 or g == h) and L[h, y, x]]
        if not named:
            rejected += 1
        for h in named:
            used.setdefault(h * n + y * ww + x, None)
    return list(used), rejected


def dijkstra(n_states, src, tgt, wgt, seeds):
    """the least weight to a seed per state over the reversed moves, candidates above MAX dropped: a list of Python ints"""
    order = np.argsort(tgt, kind="stable")
    first = np.searchsorted(tgt[order], np.arange(n_states + 1)).tolist()
    back, wb = src[order].tolist(), wgt[order].tolist()
    dist = [UNREACHED] * n_states
    heap = []
    for u in seeds:
        dist[u] = 0
        heap.append((0, u))
    heapq.heapify(heap)
    while heap:
        d, u = heapq.heappop(heap)
        if d != dist[u]:
            continue
        for k in range(first[u], first[u + 1]):
            cand = d + wb[k]
            if cand <= MAX and cand < dist[back[k]]:
                dist[back[k]] = cand
                heapq.heappush(heap, (cand, back[k]))
    return dist


def solve(geo, plane, p, footprint, goals):
    """dict(L, P uint32 (8, h, w), floor uint32 (h, w), floor_heading uint8 (h, w), summary, error).  A refused solve has
    error=True and a summary of zeros."""
    w, h = geo["width"], geo["height"]
    zero = dict.fromkeys(SUMMARY_KEYS, 0)
    goals = np.asarray(goals, np.int64).reshape(-1, 3)
    if not params_ok(p) or not footprint_ok(footprint) or len(goals) > 1 << 24:
        return dict(L=None, P=None, summary=zero, error=True)
    plane = np.asarray(plane, np.int8)
    assert plane.shape == (h, w)
    L = layers(plane, p, stencils(footprint))
    seeds, rejected = goal_states(L, goals)
    src, tgt, wgt = edges_of(L, p)
    dist = dijkstra(H * w * h, src, tgt, wgt, seeds)
    P64 = np.array(dist, np.int64)
    exceeded = int(bool(((P64[tgt] != UNREACHED) & (P64[tgt] + wgt > MAX)).any())) if len(tgt) else 0
    P = P64.astype(np.uint32).reshape(H, h, w)
    reached, passable = P != UNREACHED, L != 0
    floor = P.min(axis=0)
    heading = np.where(floor != UNREACHED, P.argmin(axis=0), 8).astype(np.uint8)     # (argmin: the first, so the least h)
    pv = plane.astype(int)
    summary = dict(states_blocked=int((~passable).sum()), states_reached=int(reached.sum()),
                   states_unreached=int((passable & ~reached).sum()), cells_reached=int((floor != UNREACHED).sum()),
                   cells_invalid=int(((pv < -1) | (pv > 100)).sum()), goals_used=len(seeds), goals_rejected=rejected,
                   range_exceeded=exceeded, max_potential=int(P[reached].max()) if reached.any() else 0)
    return dict(L=L.astype(np.uint32), P=P, floor=floor, floor_heading=heading, summary=summary, error=False)


def path(ref, p, start):
    """step 9 from one start (ix, iy, h): the list of states, [] where none is walked"""
    L, P = ref["L"].astype(np.int64), ref["P"]
    _, hh, ww = L.shape
    x, y, h = (int(v) for v in start)
    if not (0 <= x < ww and 0 <= y < hh and -1 <= h <= 7):
        return []
    if h < 0:
        h = int(ref["floor_heading"][y, x])
    if h == 8 or int(P[h, y, x]) == UNREACHED:
        return []
    out = [(x, y, h)]
    while int(P[h, y, x]) > 0:
        for m in range(MOVES):
            t = move(L, p, x, y, h, m)
            if t is not None and int(P[t[2], t[1], t[0]]) != UNREACHED and int(P[t[2], t[1], t[0]]) + t[3] == int(P[h, y, x]):
                x, y, h = t[:3]
                break
        else:
            raise AssertionError("no move down the field at %r" % ((x, y, h),))
        out.append((x, y, h))
    return out


def paths(ref, p, starts, cap):
    """(states uint16 (K, cap, 3), lengths uint32 (K,)) as lom_posefield_paths writes them: the rest of a row is 0"""
    starts = np.asarray(starts, np.int64).reshape(-1, 3)
    states, lengths = np.zeros((len(starts), cap, 3), np.uint16), np.zeros(len(starts), np.uint32)
    for k, s in enumerate(starts):
        route = path(ref, p, s)
        lengths[k] = len(route)
        if route and cap:
            head = np.array(route[:cap], np.uint16)
            states[k, :len(head)] = head
    return states, lengths


def path_weight(ref, p, route):
    """the sum of the weights of the moves of a route; every pair of states must be joined by an allowed move"""
    L = ref["L"].astype(np.int64)
    total = 0
    for a, b in zip(route, route[1:]):
        fits = [t[3] for t in (move(L, p, a[0], a[1], a[2], m) for m in range(MOVES)) if t is not None and t[:3] == tuple(b)]
        assert fits, (a, b)
        total += min(fits)
    return total


def query(geo, ref, xy, headings):
    """uint32 per point: P of the state, the floor for heading -1; UNREACHED outside the grid or for another heading"""
    xy = np.asarray(xy).reshape(-1, 2)
    out = np.full(len(xy), UNREACHED, np.uint32)
    for i, (cell, h) in enumerate(zip(N.cells_of(geo, xy, True), np.asarray(headings, np.int64).reshape(-1).tolist())):
        if cell is not None and -1 <= h <= 7:
            out[i] = ref["floor"][cell[1], cell[0]] if h < 0 else ref["P"][h, cell[1], cell[0]]
    return out
