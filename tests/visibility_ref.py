"""The visibility grid's definition (include/lidar_odometry_amd.h, "visibility grid") restated: walk() and cast() follow the
header step by step on Python integers, one beam and one viewpoint at a time; cast_fast() is the same definition over all
viewpoints and beams at once on numpy int64 arrays (every value stays below 2^25, so it is as exact), for the device
tests, whose cases would take minutes beam by beam -- tests/test_visibility_host.py holds the two equal.  select() is the
greedy selection on Python integers used as bit sets.  The direction table is an argument: the tests pass the library's."""
import numpy as np

KEEP_WINDOWS, KEEP_BEAMS = 1, 2
END_INVALID, END_EDGE, END_RANGE, END_HIT, END_UNKNOWN, END_CORNER = 0, 1, 2, 3, 4, 5
UNREACHED = 0xFFFFFFFF
MAX_VIEWPOINTS = 1 << 20
RECORD = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("valid", "<u4"), ("seen", "<u4"), ("unknown", "<u4"), ("free", "<u4"),
                   ("blocked", "<u4"), ("hits", "<u4")])
PICK = np.dtype([("k", "<u4"), ("gain", "<u4"), ("score", "<i8")])
SUMMARY_KEYS = ("viewpoints", "valid", "unknown_total", "unknown_max", "unknown_argmax")


def params(beams, range_cells, block_min=100, unknown_depth=0, flags=0):
    return dict(beams=beams, range_cells=range_cells, block_min=block_min, unknown_depth=unknown_depth, flags=flags)


def as_tuple(p):
    return (p["beams"], p["range_cells"], p["block_min"], p["unknown_depth"], p["flags"])


def params_ok(p):
    return (4 <= p["beams"] <= 8192 and 0 <= p["range_cells"] <= 254 and 1 <= p["block_min"] <= 100
            and 0 <= p["unknown_depth"] <= 65535 and p["flags"] & ~(KEEP_WINDOWS | KEEP_BEAMS) == 0)


def select_params(n, gain_weight=1, cost_shift=0, min_gain=1):
    return dict(n=n, gain_weight=gain_weight, cost_shift=cost_shift, min_gain=min_gain)


def select_tuple(s):
    return (s["n"], s["gain_weight"], s["cost_shift"], s["min_gain"])


def select_ok(s):
    return 1 <= s["n"] <= 1024 and 1 <= s["gain_weight"] <= 4096 and 0 <= s["cost_shift"] <= 31 and s["min_gain"] >= 1


def numpy_table(beams):
    """step 1 with numpy's cos and sin (the library's entries lie within 1 of these)"""
    a = 2.0 * np.pi * np.arange(beams) / beams
    return np.stack([np.rint(np.cos(a) * 32768.0), np.rint(np.sin(a) * 32768.0)], axis=1).astype(np.int32)


def window_shape(range_cells):
    """(rows, words per row) of a window"""
    side = 2 * range_cells + 1
    return side, (side + 31) // 32


def _sign(v):
    return (v > 0) - (v < 0)


def _blocks(plane, w, h, x, y, block_min):
    return 0 <= x < w and 0 <= y < h and int(plane[y][x]) >= block_min


def walk(plane, x0, y0, dx, dy, p):
    """steps 2 and 3 for one beam from a valid start cell: (the cells marked seen in order, without the start cell; d2 of
    the end cell; the reason)"""
    h, w = len(plane), len(plane[0])
    R, block_min, D = p["range_cells"], p["block_min"], p["unknown_depth"]
    ax, ay, sx, sy = abs(dx), abs(dy), _sign(dx), _sign(dy)
    i = j = unknown = 0
    x, y = x0, y0
    cells = []
    while True:
        lhs, rhs = (2 * i + 1) * ay, (2 * j + 1) * ax
        assert lhs < 1 << 32 and rhs < 1 << 32
        ni, nj, nx, ny = i, j, x, y
        if lhs <= rhs:
            ni, nx = i + 1, x + sx
        if lhs >= rhs:
            nj, ny = j + 1, y + sy
        if lhs == rhs and _blocks(plane, w, h, x + sx, y, block_min) and _blocks(plane, w, h, x, y + sy, block_min):
            return cells, i * i + j * j, END_CORNER
        if not (0 <= nx < w and 0 <= ny < h):
            return cells, i * i + j * j, END_EDGE
        if ni * ni + nj * nj > R * R:
            return cells, i * i + j * j, END_RANGE
        cells.append((nx, ny))
        i, j, x, y = ni, nj, nx, ny
        v = int(plane[y][x])
        if v >= block_min:
            return cells, i * i + j * j, END_HIT
        if v < 0:
            unknown += 1
            if D > 0 and unknown == D:
                return cells, i * i + j * j, END_UNKNOWN


def _finish(plane, vp, valid, seen, d2, reason, p):
    """records, beam words, windows, the unknown sets and the summary from the seen cells and the beams' ends"""
    h, w = plane.shape
    K, R = len(vp), p["range_cells"]
    side, wpr = window_shape(R)
    unknown_cells, blocking = plane < 0, plane >= p["block_min"]
    records = np.zeros(K, RECORD)
    windows = np.zeros((K, side, wpr), np.uint32)
    sets = []
    for k in range(K):
        x0, y0 = int(vp[k, 0]), int(vp[k, 1])
        records[k]["ix"], records[k]["iy"], records[k]["valid"] = x0, y0, int(valid[k])
        if not valid[k]:
            sets.append(0)
            continue
        s = seen[k]
        u = s & unknown_cells
        records[k]["seen"], records[k]["unknown"], records[k]["blocked"] = int(s.sum()), int(u.sum()), int((s & blocking).sum())
        records[k]["free"] = int((s & ~unknown_cells & ~blocking).sum())
        records[k]["hits"] = int((reason[k] == END_HIT).sum())
        gx0, gx1, gy0, gy1 = max(x0 - R, 0), min(x0 + R + 1, w), max(y0 - R, 0), min(y0 + R + 1, h)
        pad = np.zeros((side, wpr * 32), bool)
        pad[gy0 - (y0 - R):gy1 - (y0 - R), gx0 - (x0 - R):gx1 - (x0 - R)] = u[gy0:gy1, gx0:gx1]
        assert pad.sum() == u.sum()                                   # the seen cells lie in the window
        windows[k] = np.packbits(pad, axis=1, bitorder="little").view("<u4")
        sets.append(int.from_bytes(np.packbits(u.ravel(), bitorder="little").tobytes(), "little"))
    ok = np.nonzero(valid)[0]
    summary = dict(viewpoints=K, valid=len(ok), unknown_total=int(records["unknown"][ok].sum()), unknown_max=0, unknown_argmax=0)
    if len(ok):
        best = int(records["unknown"][ok].max())
        summary["unknown_max"], summary["unknown_argmax"] = best, int(ok[records["unknown"][ok] == best][0])
    beams = (d2.astype(np.uint32) | (reason.astype(np.uint32) << 24)).astype(np.uint32)
    return dict(records=records, beams=beams, windows=windows, sets=sets, summary=summary, error=None)


def _inputs(plane, viewpoints, p):
    plane = np.ascontiguousarray(plane, np.int8)
    vp = np.asarray(viewpoints, np.int64).reshape(-1, 2)
    if not params_ok(p) or len(vp) > MAX_VIEWPOINTS:
        return plane, vp, "refused"
    return plane, vp, None


def cast(plane, viewpoints, table, p):
    """steps 2 to 8 beam by beam on Python integers"""
    plane, vp, error = _inputs(plane, viewpoints, p)
    if error:
        return dict(error=error, summary=dict.fromkeys(SUMMARY_KEYS, 0))
    h, w = plane.shape
    K, B = len(vp), p["beams"]
    rows = plane.tolist()
    valid = np.zeros(K, bool)
    seen = np.zeros((K, h, w), bool)
    d2, reason = np.zeros((K, B), np.int64), np.zeros((K, B), np.int64)
    for k in range(K):
        x0, y0 = int(vp[k, 0]), int(vp[k, 1])
        if not (0 <= x0 < w and 0 <= y0 < h) or rows[y0][x0] >= p["block_min"]:
            continue
        valid[k] = True
        seen[k, y0, x0] = True
        for b in range(B):
            cells, d2[k, b], reason[k, b] = walk(rows, x0, y0, int(table[b][0]), int(table[b][1]), p)
            for x, y in cells:
                seen[k, y, x] = True
    return _finish(plane, vp, valid, seen, d2, reason, p)


def cast_fast(plane, viewpoints, table, p):
    """the same, every beam of every viewpoint a lane of int64 arrays; a lane leaves when its beam has ended"""
    plane, vp, error = _inputs(plane, viewpoints, p)
    if error:
        return dict(error=error, summary=dict.fromkeys(SUMMARY_KEYS, 0))
    h, w = plane.shape
    K, B, R, block_min, D = len(vp), p["beams"], p["range_cells"], p["block_min"], p["unknown_depth"]
    table = np.asarray(table, np.int64)
    inside = (vp[:, 0] >= 0) & (vp[:, 0] < w) & (vp[:, 1] >= 0) & (vp[:, 1] < h)
    valid = inside.copy()
    valid[inside] = plane[vp[inside, 1], vp[inside, 0]] < block_min
    seen = np.zeros((K, h, w), bool)
    d2, reason = np.zeros((K, B), np.int64), np.zeros((K, B), np.int64)
    kk = np.nonzero(valid)[0]
    seen[kk, vp[kk, 1], vp[kk, 0]] = True
    lane_k, lane_b = np.repeat(kk, B), np.tile(np.arange(B), len(kk))
    dx, dy = table[lane_b, 0], table[lane_b, 1]
    ax, ay, sx, sy = np.abs(dx), np.abs(dy), np.sign(dx), np.sign(dy)
    x, y = vp[lane_k, 0].copy(), vp[lane_k, 1].copy()
    i, j, unknown = np.zeros(len(lane_k), np.int64), np.zeros(len(lane_k), np.int64), np.zeros(len(lane_k), np.int64)

    def blocks(cx, cy):
        ok = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        out = np.zeros(len(cx), bool)
        out[ok] = plane[cy[ok], cx[ok]] >= block_min
        return out

    def end(lanes, why):
        d2[lane_k[lanes], lane_b[lanes]] = i[lanes] * i[lanes] + j[lanes] * j[lanes]
        reason[lane_k[lanes], lane_b[lanes]] = why

    a = np.arange(len(lane_k))
    while len(a):
        lhs, rhs = (2 * i[a] + 1) * ay[a], (2 * j[a] + 1) * ax[a]
        step_x, step_y = lhs <= rhs, lhs >= rhs
        ni, nj, nx, ny = i[a] + step_x, j[a] + step_y, x[a] + sx[a] * step_x, y[a] + sy[a] * step_y
        corner = (lhs == rhs) & blocks(x[a] + sx[a], y[a]) & blocks(x[a], y[a] + sy[a])
        edge = ~corner & ~((nx >= 0) & (nx < w) & (ny >= 0) & (ny < h))
        out_of_range = ~corner & ~edge & (ni * ni + nj * nj > R * R)
        end(a[corner], END_CORNER), end(a[edge], END_EDGE), end(a[out_of_range], END_RANGE)
        go = ~(corner | edge | out_of_range)
        a, ni, nj, nx, ny = a[go], ni[go], nj[go], nx[go], ny[go]
        i[a], j[a], x[a], y[a] = ni, nj, nx, ny
        seen[lane_k[a], ny, nx] = True
        v = plane[ny, nx]
        hit = v >= block_min
        unknown[a] += v < 0
        deep = ~hit & (v < 0) & (D > 0) & (unknown[a] == D)
        end(a[hit], END_HIT), end(a[deep], END_UNKNOWN)
        a = a[~(hit | deep)]
    return _finish(plane, vp, valid, seen, d2, reason, p)


def select(got, s, cost=None):
    """step 9 over a cast's unknown sets: PICK records in the order picked"""
    if not select_ok(s):
        return None
    sets, valid = got["sets"], got["records"]["valid"]
    picked, covered, out = set(), 0, []
    for _ in range(s["n"]):
        best = None
        for k in range(len(sets)):
            if not valid[k] or k in picked or (cost is not None and int(cost[k]) == UNREACHED):
                continue
            g = bin(sets[k] & ~covered).count("1")
            if g < s["min_gain"]:
                continue
            score = g * s["gain_weight"] - ((int(cost[k]) if cost is not None else 0) >> s["cost_shift"])
            if best is None or score > best[2]:
                best = (k, g, score)
        if best is None:
            break
        out.append(best)
        picked.add(best[0])
        covered |= sets[best[0]]
    return np.array(out, PICK) if out else np.zeros(0, PICK)
