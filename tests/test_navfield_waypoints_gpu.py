"""Line of sight and waypoints of the navigation field on the device against tests/navfield_waypoints_ref.py: counts,
lengths, waypoint bytes and the visibility bytes, all exactly equal, in the wave form and under the serial switch.  The
reference of a case -- the solve, and every line of sight it was asked for -- is computed once and shared."""
import ctypes as C
import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import navfield_waypoints_ref as Wr

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)
P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)
NEUTRAL, BETWEEN = 50, 140                              # max_cell_cost: cost byte 0 only; bytes 0 .. 30
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 31), (65, 33), (129, 65)]
LOOKAHEADS = (1, 2, 63, 64, 65, 130, 65535)
AMPLE = 1 << 13                                         # above the longest route of any scene here
LONG = 300                                              # a route above this many cells is cut with few settings only
REFS = {}


def geo_of(w, h):
    return N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)


def as_tuple(p):
    return (p["neutral"], p["factor"], p["unknown_cost"], p["max_passable"], p["flags"])


class Case:
    """a solved scene on the reference, with its lines of sight remembered"""

    def __init__(self, w, h, plane, p, goals, metres=False):
        self.w, self.h, self.plane, self.p, self.goals = w, h, plane, p, goals
        self.geo = geo_of(w, h)
        self.ref = N.solve(self.geo, plane, p, goals, metres)
        assert not self.ref["error"]
        self.c, self.P = self.ref["costs"], self.ref["P"]
        self.seen, self.routes = {}, {}

    def see(self, a, b, mcc):
        key = (a, b, mcc)
        if key not in self.seen:
            self.seen[key] = Wr.visible(self.c, self.w, self.h, a, b, mcc)
        return self.seen[key]

    def route(self, cell):
        if cell not in self.routes:
            inside = cell is not None and 0 <= cell[0] < self.w and 0 <= cell[1] < self.h
            self.routes[cell] = N.path(self.geo, self.c, self.P, cell if inside else None)
        return self.routes[cell]

    def waypoints(self, starts, mcc, W, route_cap, wp_cap, metres=False):
        cells_in = N.cells_of(self.geo, starts, metres)
        cells = np.zeros((len(cells_in), wp_cap, 2), np.uint16)
        counts, lengths = np.zeros(len(cells_in), np.uint32), np.zeros(len(cells_in), np.uint32)
        for k, s in enumerate(cells_in):
            route = self.route(s)
            lengths[k] = len(route)
            wp = Wr.shortcut(route[:route_cap], W, lambda a, b: self.see(a, b, mcc))
            counts[k] = len(wp)
            head = np.array(wp[:wp_cap], np.uint16).reshape(-1, 2)
            cells[k, :len(head)] = head
        return cells, counts, lengths


def case(key, *args, **kw):
    if key not in REFS:
        REFS[key] = Case(*args, **kw)
    return REFS[key]


def check(lom, dev, cs, starts, mcc, W, route_cap, wp_cap, metres=False, serial=(0, 1), what=None):
    want = cs.waypoints(starts, mcc, W, route_cap, wp_cap, metres)
    for s in serial:
        dev.setOption(lom.capi.NAV_OPT_TEST_SHORTCUT_SERIAL, s)
        cells, counts, lengths = dev.waypoints(starts, (mcc, W, route_cap, 0), wp_cap, metres=metres)
        tag = (what, mcc, W, route_cap, wp_cap, s)
        assert np.array_equal(lengths, want[2]), (tag, lengths, want[2])
        assert np.array_equal(counts, want[1]), (tag, counts, want[1])
        assert cells.shape == want[0].shape and cells.tobytes() == want[0].tobytes(), tag
    dev.setOption(lom.capi.NAV_OPT_TEST_SHORTCUT_SERIAL, 0)
    return want


def scenes_of(w, h):
    """name -> (plane, params, goals); the goals of diagonal_gaps lie on free ground on both sides of its wall"""
    rng = np.random.default_rng(1000 * w + h)
    rnd = S.random_plane(rng, w, h, obstacles=0.12)
    rnd[rng.random((h, w)) < 0.5] = 0                   # half the ground at the neutral cost: shortcuts at every threshold
    corners = np.array([(0, 0), (w - 1, h - 1), (w // 2, h // 2)], np.int32)
    return {
        "empty": (S.empty(w, h), P0, corners[1:2]),
        "random": (rnd, P0, corners),
        "random_unknown_passable": (rnd, P1, corners),
        "serpentine": (S.serpentine(w, h), P0, corners[:1]),
        "spiral": (S.spiral(w, h), P0, corners[:1]),
        "pocket": (S.pocket(w, h), P0, corners[:2]),
        "diagonal_gaps": (S.diagonal_gaps(w, h), P0, np.array([(w - 1, 0), (2, h - 1)], np.int32)),
    }


def starts_of(rng, cs):
    """cells all over the grid, the corners, goals, unreached cells and cells outside the grid: (short, long) by the length
    of the route"""
    w, h = cs.w, cs.h
    s = [(int(x), int(y)) for x, y in zip(rng.integers(0, w, 8), rng.integers(0, h, 8))]
    s += [(0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1)] + [tuple(int(v) for v in g) for g in cs.goals[:2]]
    s += [tuple(int(v) for v in u[::-1]) for u in np.argwhere(cs.P == N.UNREACHED)[:2]]
    outside = [(-1, 0), (w, h - 1), (0, h), (3, -7)]
    short = [c for c in s if len(cs.route(c)) <= LONG] + outside
    long = sorted((c for c in s if len(cs.route(c)) > LONG), key=lambda c: -len(cs.route(c)))[:1]
    return np.array(short, np.int32).reshape(-1, 2), np.array(long, np.int32).reshape(-1, 2)


# ---- 1: shapes x scenes x parameters x both forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_scenes_and_parameters(lom, w, h):
    rng = np.random.default_rng(w + 7 * h)
    dev = lom.NavField(RES, ORIGIN, w, h)
    cut = 0
    for name, (plane, p, goals) in scenes_of(w, h).items():
        cs = case((w, h, name), w, h, plane, p, goals)
        assert dev.solve(plane, as_tuple(p), goals) == cs.ref["summary"], name
        short, long = starts_of(rng, cs)
        for mcc in (0, NEUTRAL, BETWEEN):
            for W in LOOKAHEADS:
                want = check(lom, dev, cs, short, mcc, W, AMPLE, 48, what=name)
                if W == 1:                                               # the route itself, whatever the threshold
                    assert np.array_equal(want[1], want[2])
                cut += int((want[1] < want[2]).sum())
        for route_cap in (1, 2, 40):
            for wp_cap in (0, 1, 3):
                check(lom, dev, cs, short, (0, NEUTRAL, BETWEEN)[wp_cap % 3], (64, 2, 65535)[route_cap % 3], route_cap, wp_cap, what=name)
        if len(long):
            for mcc, W, route_cap in ((0, 64, AMPLE), (BETWEEN, 2, AMPLE), (0, 65535, 40)):
                want = check(lom, dev, cs, long, mcc, W, route_cap, AMPLE if W == 2 else 100, what=(name, "long"))
                assert want[2][0] > LONG
        pairs = np.stack([rng.integers(-1, w + 1, 120), rng.integers(-1, h + 1, 120), rng.integers(-1, w + 1, 120),
                          rng.integers(-1, h + 1, 120)], axis=1).astype(np.int32)
        for mcc in (0, NEUTRAL, BETWEEN):
            assert np.array_equal(dev.visible(pairs, mcc), Wr.visible_many(cs.c, w, h, pairs, mcc)), (name, mcc)
    if (w, h) == (129, 65):
        assert cut > 100                                                 # shortcuts were taken
        assert any(len(r) > 2000 for r in REFS[(w, h, "serpentine")].routes.values())


def test_starts_in_metres(lom):
    w, h = 65, 33
    rng = np.random.default_rng(3)
    plane = S.random_plane(rng, w, h, obstacles=0.08)
    plane[rng.random((h, w)) < 0.5] = 0
    goals = np.array([[4.9, 6.1], [-2.9, 2.1], [np.nan, 5.0]], np.float32)
    plane[16, 31] = plane[0, 0] = 0                                      # the cells of the first two
    cs = case("metres", w, h, plane, P1, goals, metres=True)
    dev = lom.NavField(RES, ORIGIN, w, h)
    assert dev.solve(plane, as_tuple(P1), goals, metres=True) == cs.ref["summary"] and cs.ref["summary"]["goals_used"] == 2
    nan, inf = np.nan, np.inf
    xy = np.concatenate([np.array([[-3.0, 2.0], [-2.75, 2.25], [-2.7500002, 2.2499998], [13.249999, 10.249999], [13.25, 5.0], [5.0, 10.25],
                                   [-3.0000002, 5.0], [nan, 5.0], [5.0, -inf], [4.9, 6.1], [1e30, -1e30]], np.float32),
                         rng.uniform(-5, 15, (40, 2)).astype(np.float32)])
    for mcc, W in ((0, 65535), (NEUTRAL, 64), (BETWEEN, 3)):
        want = check(lom, dev, cs, xy, mcc, W, AMPLE, 40, metres=True)
        assert (want[1][6:9] == 0).all() and want[1][9] == 1 and (want[1] > 1).sum() > 10
    # the mirrors of the output: cell centres in metres, the length of a polyline
    cells, counts, lengths = dev.waypoints(xy, (0, 65535, AMPLE, 0), 40, metres=True)
    k = int(np.argmax(counts))
    m = dev.waypointsMetres(cells[k, :counts[k]])
    assert np.array_equal(m, np.array(ORIGIN) + (cells[k, :counts[k]].astype(np.float64) + 0.5) * RES)
    route = dev.paths(xy[k:k + 1], int(lengths[k]), metres=True)[0][0]
    assert dev.polylineLength(cells[k], counts[k]) == pytest.approx(Wr.polyline_cells(cells[k, :counts[k]]) * RES, rel=1e-12)
    assert dev.polylineLength(cells[k], counts[k]) <= dev.polylineLength(route) + 1e-9


# ---- 2: chunk edges ------------------------------------------------------------------------------------------------------------
def test_chunk_edges_on_open_ground(lom):
    """A straight route of 129 cells along row 30 of (129, 65) `empty`, and one cell of it that is not clear under
    max_cell_cost = neutral (cost byte 10: the route still runs through it, a detour costs more).  From the start exactly
    the cells in front of that cell are visible, so the cell chooses which lane of which chunk holds the greatest visible
    candidate: the farthest lane of the farthest chunk (no such cell), its nearest lane, the farthest lane of the nearest
    chunk, the nearest tested lane of the nearest chunk (a + 2), and a + 1 alone."""
    w, h, y = 129, 65, 30
    dev = lom.NavField(RES, ORIGIN, w, h)
    goals, start = np.array([(128, y)], np.int32), np.array([(0, y)], np.int32)
    for costly in (None, 66, 65, 64, 3, 2):
        plane = S.empty(w, h)
        if costly is not None:
            plane[y, costly] = 10
        cs = case(("edge", costly), w, h, plane, P0, goals)
        assert cs.route((0, y)) == [(x, y) for x in range(129)]
        assert dev.solve(plane, as_tuple(P0), goals) == cs.ref["summary"]
        for W in (1, 2, 63, 64, 65, 127, 128, 129, 130, 65535):
            want = check(lom, dev, cs, start, NEUTRAL, W, AMPLE, 140, what=("edge", costly))
            first = min(W, 128) if costly is None else min(W, costly - 1)
            assert tuple(want[0][0, 1]) == (first, y), (costly, W)
            check(lom, dev, cs, start, 0, W, AMPLE, 140, what=("edge", costly, "any cost"))
    # a blocked cell east of the start: every route cell but a + 1 lies in its shadow, from the start nothing is visible
    plane = S.empty(w, h)
    plane[y, 11] = 100
    cs = case(("edge", "blocked"), w, h, plane, P0, goals)
    assert dev.solve(plane, as_tuple(P0), goals) == cs.ref["summary"]
    s = np.array([(10, y)], np.int32)
    route = cs.route((10, y))
    assert not any(cs.see((10, y), b, 0) for b in route[2:])
    for W in (2, 64, 65535):
        want = check(lom, dev, cs, s, 0, W, AMPLE, 140, what="shadow")
        assert tuple(want[0][0, 1]) == route[1]


@pytest.mark.parametrize("scene", ["empty", "serpentine"])
def test_routes_of_64_to_130_cells(lom, scene):
    """routes one cell either side of one and of two full chunks.  On `empty` a route has at most 129 cells; the serpentine's
    corridor gives all five lengths, the last one round its first bend."""
    w, h = 129, 65
    plane = S.empty(w, h) if scene == "empty" else S.serpentine(w, h)
    goals = np.array([(0, 0)], np.int32)
    cs = case(("lengths", scene), w, h, plane, P0, goals)
    dev = lom.NavField(RES, ORIGIN, w, h)
    assert dev.solve(plane, as_tuple(P0), goals) == cs.ref["summary"]
    starts = [(63, 0), (64, 0), (65, 0), (128, 0), (128, 1), (63, 40), (64, 64), (128, 64)]
    if scene == "serpentine":
        starts = starts[:5]
        assert [len(cs.route(s)) for s in starts] == [64, 65, 66, 129, 130]
    else:
        assert [len(cs.route(s)) for s in starts[:4]] == [64, 65, 66, 129]
    starts = np.array(starts, np.int32)
    for W in (63, 64, 65, 128, 129, 65535):
        for mcc in (0, NEUTRAL):
            check(lom, dev, cs, starts, mcc, W, AMPLE, 16, what=scene)
            check(lom, dev, cs, starts, mcc, W, 65, 16, what=scene)


# ---- 3: long segments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(8192, 3), (3, 8192)])
def test_visible_along_the_longest_grid(lom, w, h):
    dev = lom.NavField(RES, ORIGIN, w, h)
    flip = (lambda c: c) if w > h else (lambda c: (c[1], c[0]))
    ends = [((0, 0), (8191, 2)), ((8191, 0), (0, 2)), ((0, 2), (8191, 0)), ((8191, 2), (0, 0)), ((0, 1), (8191, 1)), ((8191, 1), (0, 1))]
    pairs = np.array([flip(a) + flip(b) for a, b in ends], np.int32)
    none = np.zeros((0, 2), np.int32)
    seen = []
    for blocked in (None, (1, 0), (4096, 1), (8190, 2), (8190, 0)):
        plane = S.empty(w, h)
        if blocked is not None:
            bx, by = flip(blocked)
            plane[by, bx] = 100
        dev.solve(plane, as_tuple(P0), none)
        want = Wr.visible_many(N.costs_of(plane, P0), w, h, pairs, 0)
        got = dev.visible(pairs, 0)
        assert np.array_equal(got, want), (blocked, got, want)
        seen.append(want.tolist())
    assert seen[0] == [1] * 6 and seen[1] == [0, 1, 1, 0, 1, 1] and seen[2] == [0] * 6 and seen[3] == [0, 1, 1, 0, 1, 1]
    assert seen[4] == [1, 0, 0, 1, 1, 1]


def test_visible_on_a_large_grid(lom):
    w = h = 1024
    rng = np.random.default_rng(11)
    plane = np.where(rng.random((h, w)) < 0.002, 100, np.where(rng.random((h, w)) < 0.06, 20, 0)).astype(np.int8)
    dev = lom.NavField(RES, ORIGIN, w, h)
    dev.solve(plane, as_tuple(P0), np.zeros((0, 2), np.int32))
    a = rng.integers(0, w, (300, 2))
    far = rng.integers(0, w, (300, 2))
    near = np.clip(a + rng.integers(-12, 13, (300, 2)), -2, w + 1)
    pairs = np.concatenate([np.concatenate([a, far], axis=1)[:150], np.concatenate([a, near], axis=1)[150:]]).astype(np.int32)
    t = np.array(N.cell_costs(P0), np.int64)
    c = t[plane.view(np.uint8)].tolist()
    for mcc in (0, NEUTRAL):
        want = Wr.visible_many(c, w, h, pairs, mcc)
        assert np.array_equal(dev.visible(pairs, mcc), want), mcc
        assert 20 < int(want.sum()) < 280
    assert len(dev.visible(np.zeros((0, 4), np.int32))) == 0


# ---- 4: purity, refusals, the handle's states ------------------------------------------------------------------------------------
def test_two_runs_agree_and_a_refused_call_writes_nothing(lom):
    w, h = 65, 33
    rng = np.random.default_rng(30)
    plane = S.random_plane(rng, w, h, obstacles=0.1)
    plane[rng.random((h, w)) < 0.5] = 0
    goals = np.array([(0, 0), (w - 1, h - 1)], np.int32)
    cs = case("purity", w, h, plane, P1, goals)
    dev = lom.NavField(RES, ORIGIN, w, h)
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    # no solve yet: no start is walked, only a cell itself is visible; not a state error
    starts, _ = starts_of(rng, cs)
    cells, counts, lengths = dev.waypoints(starts, (0, 64, 100, 0), 5)
    assert not cells.any() and not counts.any() and not lengths.any()
    assert dev.visible(np.array([(3, 3, 3, 3), (3, 3, 4, 3), (-1, 0, -1, 0)], np.int32)).tolist() == [1, 0, 0]
    dev.solve(plane, as_tuple(P1), goals)
    first = dev.waypoints(starts, (NEUTRAL, 64, 100, 0), 20)
    dev.waypoints(starts[::-1].copy(), (0, 3, 7, 0), 2)                  # another call in between, on the same buffers
    dev.paths(starts, 3)
    again = dev.waypoints(starts, (NEUTRAL, 64, 100, 0), 20)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    want = cs.waypoints(starts, NEUTRAL, 64, 100, 20)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, want))
    # refusals: nothing is written
    s32 = np.ascontiguousarray(starts, np.int32)
    cells, counts, lengths = np.full((len(s32), 4, 2), 7, np.uint16), np.full(len(s32), 7, np.uint32), np.full(len(s32), 7, np.uint32)
    good = lom.navfieldWaypointParams((NEUTRAL, 64, 100, 0))

    def call(kind=0, pts=s32.ctypes.data, n=len(s32), prm=good, out=cells.ctypes.data, cap=4):
        return L.lom_navfield_waypoints(dev.handle, kind, pts, n, None if prm is None else C.byref(prm), out, cap, counts.ctypes.data,
                                        lengths.ctypes.data)

    for bad in ((0, 0, 100, 0), (0, 65536, 100, 0), (0, 64, 0, 0), (0, 64, 100, 1), (0, 64, 100, 0x80000000), (0, 64, (1 << 28) // len(s32) + 1, 0)):
        assert call(prm=lom.navfieldWaypointParams(bad)) == ERR_ARG, bad
        assert L.lom_navfield_last_error(dev.handle)
    assert call(prm=None) == ERR_ARG and call(kind=2) == ERR_ARG and call(pts=None) == ERR_ARG and call(out=None) == ERR_ARG
    assert call(n=(1 << 24) + 1) == ERR_ARG and call(cap=(1 << 28) // len(s32) + 1) == ERR_ARG
    out, q = np.full(3, 7, np.uint8), np.zeros((3, 4), np.int32)
    assert L.lom_navfield_visible(dev.handle, None, 3, 0, out.ctypes.data) == ERR_ARG
    assert L.lom_navfield_visible(dev.handle, q.ctypes.data, 3, 0, None) == ERR_ARG
    assert L.lom_navfield_visible(dev.handle, q.ctypes.data, (1 << 24) + 1, 0, out.ctypes.data) == ERR_ARG
    assert (cells == 7).all() and (counts == 7).all() and (lengths == 7).all() and (out == 7).all()
    with pytest.raises(lom.LomError):
        dev.setOption(lom.capi.NAV_OPT_TEST_SHORTCUT_SERIAL, 2)
    # the optional outputs, and no start at all
    assert call(out=None, cap=0) == 0 and counts.tolist() == want[1].tolist() and lengths.tolist() == want[2].tolist()
    assert L.lom_navfield_waypoints(dev.handle, 0, s32.ctypes.data, len(s32), C.byref(good), None, 0, None, None) == 0
    cells, counts, lengths = dev.waypoints(np.zeros((0, 2), np.int32), (0, 64, 100, 0), 5)
    assert cells.shape == (0, 5, 2) and len(counts) == 0 and len(lengths) == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dev.waypoints(starts, (NEUTRAL, 64, 100, 0), 20), want))
    dev.clear()
    assert not dev.waypoints(starts, (0, 64, 100, 0), 5)[1].any()


def test_waypoints_after_a_resolve(lom):
    w, h = 65, 33
    rng = np.random.default_rng(41)
    plane = S.random_plane(rng, w, h, obstacles=0.08)
    plane[rng.random((h, w)) < 0.5] = 0
    goals = np.array([(1, 14)], np.int32)                                # every route from the right crosses the window
    plane[14, 1] = 0
    new = plane.copy()
    new[8:20, 20:24] = 100                                               # a wall across the window, and cheaper ground beside it
    new[8:20, 30:40] = 0
    window = (18, 6, 24, 16)
    merged = plane.copy()
    merged[6:22, 18:42] = new[6:22, 18:42]
    cs = case("resolve", w, h, merged, P1, goals)
    dev = lom.NavField(RES, ORIGIN, w, h)
    dev.solve(plane, as_tuple(P1), goals)
    starts, _ = starts_of(rng, cs)
    before = dev.waypoints(starts, (0, 64, AMPLE, 0), 30)
    assert dev.resolve(new, window) == cs.ref["summary"]
    for mcc, W in ((0, 64), (NEUTRAL, 65535)):
        want = check(lom, dev, cs, starts, mcc, W, AMPLE, 30, what="resolve")
    assert before[0].tobytes() != dev.waypoints(starts, (0, 64, AMPLE, 0), 30)[0].tobytes()


def test_the_chain_from_the_clearance_grid(lom):
    """ClearanceGrid -> NavField.solveFromClearance -> waypoints with max_cell_cost = neutral, which keeps every shortcut
    outside the inflation radius, against the references' chain"""
    rng = np.random.default_rng(21)
    w, h = 130, 67
    occ = np.where(rng.random((h, w)) < 0.006, 100, 0).astype(np.int8)
    occ[30:34, 40:90] = 100
    cp = K.params(1.0, 0.3, 1.5)
    clear = lom.ClearanceGrid(RES, ORIGIN, w, h)
    clear.update(occ, None, cp)
    cost = K.update(K.geometry(RES, ORIGIN[0], ORIGIN[1], w, h), occ, None, cp)["cost"]
    assert clear.cost()[0].tobytes() == cost.tobytes() and (cost == 0).sum() > 1000 and ((cost > 0) & (cost < 99)).any()
    goals = np.array([(w - 3, h - 3), (2, 2)], np.int32)
    cost_at_goals = [int(cost[y, x]) for x, y in goals]
    assert max(cost_at_goals) < 99
    cs = case("chain", w, h, cost, P0, goals)
    dev = lom.NavField(RES, ORIGIN, w, h)
    assert dev.solveFromClearance(clear, as_tuple(P0), goals) == cs.ref["summary"]
    starts, _ = starts_of(rng, cs)
    for mcc, W in ((NEUTRAL, 65535), (NEUTRAL, 64), (0, 65535)):
        want = check(lom, dev, cs, starts, mcc, W, AMPLE, 60, what="chain")
        assert (want[1] < want[2]).sum() > 5
    # under max_cell_cost = neutral every cell a shortcut crosses has cost byte 0
    cells, counts, _ = dev.waypoints(starts, (NEUTRAL, 65535, AMPLE, 0), 60)
    for k in range(len(starts)):
        route = cs.route(N.cells_of(cs.geo, starts[k:k + 1], False)[0])
        at = [route.index(tuple(int(v) for v in c)) for c in cells[k, :counts[k]]]
        for i, j in zip(at, at[1:]):
            if j - i > 1:
                assert Wr.visible_by_fractions(cs.c, w, h, route[i], route[j], NEUTRAL)


# ---- mirrors -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::NavField::waypoints and ::visible of the C++ mirror compile with plain g++ and leave the bytes the Python package
    leaves."""
    exe = cpp_program.build_with_library(tmp_path, "test_navfield_waypoints_mirror.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    lines = stdout.strip().split("\n")
    got = [np.array([int(v) for v in line.split()], np.int64) for line in lines[-4:]]
    # the same grid, plane, goal, starts and pairs here (tests/cpp/test_navfield_waypoints_mirror.cpp)
    w, h, wp_cap = 45, 37, 64
    i = np.arange(w * h)
    plane = np.where(i % 7 == 3, 100, (i % 4) * 5).astype(np.int8).reshape(h, w)
    p = N.params(20, 2, 300, 80)
    goals = np.array([(40, 30)], np.int32)
    starts = np.array([(0, 0), (44, 0), (40, 30), (-1, 2), (2, 36)], np.int32)
    k = np.arange(60)
    pairs = np.stack([(k * 7) % 45, (k * 5) % 37, ((k * 7) % 45 + k % 5) % 45, ((k * 5) % 37 + k % 3) % 37], axis=1).astype(np.int32)
    dev = lom.NavField(RES, ORIGIN, w, h)
    dev.solve(plane, as_tuple(p), goals)
    cells, counts, lengths = dev.waypoints(starts, (40, 64, 200, 0), wp_cap)
    vis = dev.visible(pairs, 40)
    assert got[0].tolist() == counts.tolist() and got[1].tolist() == lengths.tolist()
    assert got[2].astype(np.uint16).tobytes() == cells.tobytes() and got[3].astype(np.uint8).tobytes() == vis.tobytes()
    cs = Case(w, h, plane, p, goals)
    want = cs.waypoints(starts, 40, 64, 200, wp_cap)
    assert cells.tobytes() == want[0].tobytes() and counts.tolist() == want[1].tolist() and lengths.tolist() == want[2].tolist()
    assert vis.tolist() == Wr.visible_many(cs.c, w, h, pairs, 40).tolist() and 0 < vis.sum() < 60 and (counts[[0, 1, 4]] < lengths[[0, 1, 4]]).all()
