"""The navigation field set on the device against tests/navset_ref.py and against NavField on the device: every field as
bytes and every summary exactly equal, under the three test switches; gather, nearest, paths, adopt, the forms of a solve,
the chain to the rollouts, shift, refusals.  No tolerance anywhere: a field is the unique fixed point of its relaxation.  The
reference of a field is computed once per (shape, scene, goals) and shared.

What a set of n_fields is solved under: all eight settings of the switches at n_fields = 5 (every kind of field is in it);
the other counts take one setting each, rotated with the scene, so that every count meets every setting over the scenes
of a shape.  No test asserts a time or a launch count."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import navset_ref as NS
from tests import rollout_ref as R
from tests.rollout_scenes import commands_of, states_of

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)
P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)
SHAPES = [(1, 1), (1, 70), (70, 1), (32, 32), (33, 31), (65, 33), (129, 65)]
# inner cap (0: the default), launches per wait, all tiles
SWITCHES = [(cap, batch, every) for cap in (1, 0) for batch in (1, 8) for every in (0, 1)]
COUNTS = (0, 1, 2, 5, 17)
REFS = {}


def geo_of(w, h):
    return N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)


def as_tuple(p):
    return (p["neutral"], p["factor"], p["unknown_cost"], p["max_passable"], p["flags"])


def reference(key, w, h, plane, p, goals, metres=False):
    """the reference's solve of one field, once per (key, goals)"""
    key = (key, np.asarray(goals).tobytes(), metres)
    if key not in REFS:
        REFS[key] = N.solve(geo_of(w, h), plane, p, goals, metres)
    return REFS[key]


def references(key, w, h, plane, p, goals_per_field):
    return [reference(key, w, h, plane, p, g) for g in goals_per_field]


def set_switches(lom, dev, cap, batch, every):
    dev.setOption(lom.capi.NAVSET_OPT_TEST_INNER_CAP, cap)
    dev.setOption(lom.capi.NAVSET_OPT_TEST_BATCH, batch)
    dev.setOption(lom.capi.NAVSET_OPT_TEST_ALL_TILES, every)


def border_goals(w, h):
    """the four corners, cells on both sides of every tile border, duplicates, and goals outside the grid"""
    g = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (0, 0), (w - 1, h - 1)]
    for v in (31, 32, 63, 64):
        g += [(v, h // 2), (w // 2, v), (v, v)]
    g += [(-1, 0), (0, -1), (w, 0), (0, h), (w + 5, h + 5), (-(2 ** 31), 2 ** 31 - 1)]
    return np.array(g, np.int64).astype(np.int32)


def fields_of(rng, w, h, plane):
    """17 goal lists.  0: the border goals; 1: none; 2: only rejected or outside goals; 3: one far corner; 4: identical to
    0; 5: shares the corner with 3; then one to three random cells each, free ones where there are any."""
    blocked = np.argwhere(plane == 100)[:2, ::-1]
    outside = np.array([(-1, 0), (w, h), (0, h), (-(2 ** 31), 5)], np.int64)
    far = np.array([(w - 1, h - 1)], np.int64)
    free = np.argwhere((plane >= 0) & (plane <= 90))[:, ::-1]
    pool = free if len(free) else np.array([(0, 0)])
    out = [border_goals(w, h), np.zeros((0, 2), np.int32), np.concatenate([outside, blocked]), far, border_goals(w, h),
           np.concatenate([far, [(0, h - 1)]])]
    while len(out) < 17:
        out.append(pool[rng.integers(0, len(pool), 1 + len(out) % 3)])
    return [np.asarray(g, np.int64).astype(np.int32).reshape(-1, 2) for g in out]


def scenes_of(w, h):
    """name -> (plane, params)"""
    rng = np.random.default_rng(1000 * w + h)
    rnd = S.random_plane(rng, w, h)
    return {"empty": (S.empty(w, h), P0), "random": (rnd, P0), "random_unknown_passable": (rnd, P1), "serpentine": (S.serpentine(w, h), P0),
            "spiral": (S.spiral(w, h), P0), "diagonal_gaps": (S.diagonal_gaps(w, h), P0), "pocket": (S.pocket(w, h), P0),
            "all_blocked": (np.full((h, w), 100, np.int8), P0)}


def check_set(dev, refs, plane, p, goals, what=None):
    """one solve of a set against the references of its fields"""
    summaries = dev.solve(plane, as_tuple(p), goals)
    assert dev.fieldCount() == len(goals) == len(summaries), what
    for i, ref in enumerate(refs):
        got = dev.potential(i)
        assert got.tobytes() == ref["P"].tobytes(), (what, i, np.argwhere(got != ref["P"])[:10])
        assert summaries[i] == ref["summary"], (what, i, summaries[i], ref["summary"])
    st = dev.stats()
    assert st["fields"] == len(goals)
    if goals:
        assert st["launches"] >= 1 and 1 <= st["waits"] <= st["launches"]


# ---- 1: shapes x scenes x field counts x switches ----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_scenes_counts_and_switches(lom, w, h):
    dev, single = lom.NavFieldSet(RES, ORIGIN, w, h, 17), lom.NavField(RES, ORIGIN, w, h)
    for k, (name, (plane, p)) in enumerate(scenes_of(w, h).items()):
        rng = np.random.default_rng(w + 7 * h + k)
        fields = fields_of(rng, w, h, plane)
        # 17 fields at the largest shape on two scenes only
        counts = COUNTS if (w, h) != SHAPES[-1] or name in ("random_unknown_passable", "spiral") else COUNTS[:-1]
        for j, n in enumerate(counts):
            goals = fields[:n]
            refs = references((w, h, name), w, h, plane, p, goals)
            assert not any(r["error"] for r in refs)
            for cap, batch, every in (SWITCHES if n == 5 else [SWITCHES[(j + k) % len(SWITCHES)]]):
                set_switches(lom, dev, cap, batch, every)
                check_set(dev, refs, plane, p, goals, what=(name, n, cap, batch, every))
        # ... and a NavField.solve on the device gives the same bytes and summary, field by field
        set_switches(lom, dev, 0, 0, 0)
        goals = fields[:counts[-1]]
        summaries = dev.solve(plane, as_tuple(p), goals)
        for i, g in enumerate(goals):
            if i in (0, 1, 2, 3, 5, 6, 11, 16):
                assert single.solve(plane, as_tuple(p), g) == summaries[i], (name, i)
                assert single.potential().tobytes() == dev.potential(i).tobytes(), (name, i)
    # what the field mixes are for, on the reference
    if (w, h) == (129, 65):
        plane, p = scenes_of(w, h)["random"]
        refs = references((w, h, "random"), w, h, plane, p, fields_of(np.random.default_rng(w + 7 * h + 1), w, h, plane)[:6])
        assert refs[0]["summary"]["goals_rejected"] > 6 and refs[0]["summary"]["goals_used"] >= 2
        assert refs[1]["summary"]["cells_reached"] == 0 and refs[1]["summary"]["goals_used"] == 0
        assert refs[2]["summary"]["goals_used"] == 0 and refs[2]["summary"]["goals_rejected"] == 6 and refs[2]["summary"]["cells_reached"] == 0
        plane, p = scenes_of(w, h)["empty"]
        refs = references((w, h, "empty"), w, h, plane, p, fields_of(np.random.default_rng(w + 7 * h), w, h, plane)[:6])
        assert refs[4]["P"].tobytes() == refs[0]["P"].tobytes() and refs[5]["P"].tobytes() != refs[3]["P"].tobytes()
        assert refs[5]["P"][h - 1, w - 1] == refs[3]["P"][h - 1, w - 1] == 0


def test_goals_in_metres(lom):
    w, h = 65, 33
    plane = S.random_plane(np.random.default_rng(3), w, h, obstacles=0.1)
    nan, inf = np.nan, np.inf
    goals = [np.array([[-3.0, 2.0], [-2.75, 2.25], [-2.7500002, 2.2499998], [nan, 5.0], [4.9, 6.1], [4.9, 6.1]], np.float32),
             np.array([[13.249999, 10.249999], [13.25, 5.0], [5.0, 10.25], [-3.0000002, 5.0], [inf, 5.0], [1e30, -1e30]], np.float32),
             np.zeros((0, 2), np.float32)]
    refs = [reference("metres", w, h, plane, P1, g, metres=True) for g in goals]
    assert refs[0]["summary"]["goals_rejected"] >= 1 and refs[1]["summary"]["goals_rejected"] >= 5
    dev = lom.NavFieldSet(RES, ORIGIN, w, h, 3)
    summaries = dev.solve(plane, as_tuple(P1), goals, metres=True)
    for i, ref in enumerate(refs):
        assert dev.potential(i).tobytes() == ref["P"].tobytes() and summaries[i] == ref["summary"], i


# ---- 2: gather ---------------------------------------------------------------------------------------------------------------
def test_gather_in_cells_in_metres_outside_and_none(lom):
    w, h = 65, 33
    rng = np.random.default_rng(11)
    plane, geo = S.random_plane(rng, w, h, obstacles=0.15), geo_of(w, h)
    goals = fields_of(rng, w, h, plane)[:7]
    refs = references("gather", w, h, plane, P1, goals)
    dev = lom.NavFieldSet(RES, ORIGIN, w, h, 8)
    assert dev.gather(np.array([(0, 0)], np.int32)).shape == (0, 1)                  # before any solve: no fields
    dev.solve(plane, as_tuple(P1), goals)
    cells = np.concatenate([np.stack([rng.integers(0, w, 300), rng.integers(0, h, 300)], axis=1),
                            [(-1, 0), (w, 0), (0, h), (0, -1), (w + 9, h + 9), (-(2 ** 31), 2 ** 31 - 1), (0, 0), (w - 1, h - 1)]]).astype(np.int32)
    want = NS.gather(geo, refs, cells)
    assert dev.gather(cells).tobytes() == want.tobytes() and (want[:, 300:306] == N.UNREACHED).all() and (want != N.UNREACHED).sum() > 500
    xy = np.concatenate([rng.uniform(ORIGIN[0] - 1.0, ORIGIN[0] + w * RES + 1.0, (300, 1)), rng.uniform(ORIGIN[1] - 1.0, ORIGIN[1] + h * RES + 1.0, (300, 1))],
                        axis=1).astype(np.float32)
    xy = np.concatenate([xy, np.array([[-3.0, 2.0], [-3.0000002, 2.0], [13.249999, 10.249999], [13.25, 10.25], [np.nan, 3.0], [3.0, np.inf]], np.float32)])
    want = NS.gather(geo, refs, xy, metres=True)
    assert dev.gather(xy, metres=True).tobytes() == want.tobytes() and (want[:, -2:] == N.UNREACHED).all()
    assert dev.gather(np.zeros((0, 2), np.int32)).shape == (7, 0)
    # with the goals as the points: the travel-cost matrix, zero on its diagonal where the goal was used
    at = np.array([g[0] for g in goals[6:7] * 3], np.int32)
    m = dev.gather(at)
    assert m.shape == (7, 3) and (m[6] == 0).all()


def test_the_matrix_is_not_symmetric_over_a_costly_cell(lom):
    plane = np.zeros((1, 6), np.int8)
    plane[0, 4] = 60
    a, b = (1, 0), (4, 0)
    dev = lom.NavFieldSet(RES, ORIGIN, 6, 1, 2)
    dev.solve(plane, as_tuple(P0), [np.array([a]), np.array([b])])
    m = dev.gather(np.array([a, b], np.int32))
    assert m.tolist() == [[0, 5 * 230 + 2 * 5 * 50], [3 * 5 * 50, 0]]


# ---- 3: nearest --------------------------------------------------------------------------------------------------------------
def test_nearest_with_ties_and_the_union_invariant(lom):
    L = lom.capi.lib()
    for w, h, plane, p, goals in (
            # a free plane and mirrored goals: whole rows and diagonals of equal values, which go to the least index
            (65, 33, S.empty(65, 33), P0, [np.array([(0, 16)]), np.array([(64, 16)]), np.array([(32, 0)]), np.array([(32, 32)]), np.array([(0, 16)])]),
            (129, 65, S.random_plane(np.random.default_rng(5), 129, 65), P1, None),
            (33, 31, S.pocket(33, 31), P0, [np.zeros((0, 2), np.int32), np.array([(0, 0), (32, 30)]), np.array([(16, 15)])]),
            (70, 1, S.empty(70, 1), P0, [np.array([(69, 0)]), np.array([(0, 0)])])):
        if goals is None:
            goals = fields_of(np.random.default_rng(6), w, h, plane)
        goals = [np.asarray(g, np.int32).reshape(-1, 2) for g in goals]
        refs = references(("nearest", w, h), w, h, plane, p, goals)
        want_owner, want_p, want_owned = NS.nearest(geo_of(w, h), refs)
        dev = lom.NavFieldSet(RES, ORIGIN, w, h, 17)
        dev.solve(plane, as_tuple(p), goals)
        owner, potential, owned = dev.nearest()
        assert owner.tobytes() == want_owner.tobytes() and potential.tobytes() == want_p.tobytes()
        assert np.array_equal(owned, want_owned) and int(owned.sum()) == int((want_owner != NS.NO_OWNER).sum())
        # the invariant: the potential is the single solve from the union of all goals
        single = lom.NavField(RES, ORIGIN, w, h)
        single.solve(plane, as_tuple(p), np.concatenate(goals))
        assert single.potential().tobytes() == potential.tobytes()
        # each output alone
        only = np.zeros(len(goals), np.uint64)
        assert L.lom_navset_nearest(dev.handle, None, None, only.ctypes.data) == 0 and np.array_equal(only, want_owned)
        assert L.lom_navset_nearest(dev.handle, None, None, None) == 0
        if (w, h) == (65, 33):                        # ties did occur, and a duplicate of field 0 owns nothing
            stack = np.stack([r["P"] for r in refs[:4]])
            assert ((stack == want_p).sum(axis=0) >= 2).sum() >= 33 and owned[4] == 0 and (owned[:4] > 0).all()
    # no fields: nobody owns anything
    dev = lom.NavFieldSet(RES, ORIGIN, 33, 31, 4)
    with pytest.raises(lom.LomError) as e:
        dev.nearest()
    assert e.value.code == lom.capi.ERR_STATE
    dev.solve(S.empty(33, 31), as_tuple(P0), [])
    owner, potential, owned = dev.nearest()
    assert (owner == NS.NO_OWNER).all() and (potential == N.UNREACHED).all() and len(owned) == 0


# ---- 4: paths ----------------------------------------------------------------------------------------------------------------
def test_paths_across_fields_and_their_refusal(lom):
    w, h = 65, 33
    rng = np.random.default_rng(13)
    plane, geo = S.random_plane(rng, w, h, obstacles=0.15), geo_of(w, h)
    goals = fields_of(rng, w, h, plane)[:6]
    refs = references("paths", w, h, plane, P1, goals)
    dev = lom.NavFieldSet(RES, ORIGIN, w, h, 6)
    dev.solve(plane, as_tuple(P1), goals)
    starts = np.concatenate([np.stack([rng.integers(0, w, 40), rng.integers(0, h, 40)], axis=1), [(0, 0), (w - 1, h - 1), (-1, 0), (w, h - 1), (3, -7)]]).astype(np.int32)
    which = rng.integers(0, 6, len(starts)).astype(np.int32)
    for cap in (40, 1, 0):
        cells, lengths = dev.paths(which, starts, cap)
        want_cells, want_lengths = NS.paths(geo, refs, which, starts, cap)
        assert np.array_equal(lengths, want_lengths) and cells.tobytes() == want_cells.tobytes(), cap
    assert (want_lengths > 1).sum() > 10 and (want_lengths[which == 1] == 0).all()
    xy = (np.array(ORIGIN) + (starts + 0.5) * RES).astype(np.float32)
    cells, lengths = dev.paths(which, xy, 40, metres=True)
    want_cells, want_lengths = NS.paths(geo, refs, which, xy, 40, metres=True)
    assert np.array_equal(lengths, want_lengths) and cells.tobytes() == want_cells.tobytes()
    assert dev.paths(np.zeros(0, np.int32), np.zeros((0, 2), np.int32), 5)[1].shape == (0,)
    # an index outside the fields: refused, nothing written
    L = lom.capi.lib()
    for bad in (6, -1, 2 ** 31 - 1):
        wrong = which.copy()
        wrong[7] = bad
        assert NS.paths(geo, refs, wrong, starts, 4) is None
        cells, lengths = np.full((len(starts), 4, 2), 7, np.uint16), np.full(len(starts), 7, np.uint32)
        rc = L.lom_navset_paths(dev.handle, wrong.ctypes.data, lom.capi.NAV_CELLS, starts.ctypes.data, len(starts), cells.ctypes.data, 4, lengths.ctypes.data)
        assert rc == lom.capi.ERR_ARG and (cells == 7).all() and (lengths == 7).all()


# ---- 5: adopt ----------------------------------------------------------------------------------------------------------------
def test_adopt_leaves_what_the_direct_solve_leaves(lom):
    w, h = 129, 65
    rng = np.random.default_rng(17)
    plane = S.random_plane(rng, w, h, obstacles=0.12)
    changed = plane.copy()
    changed[20:40, 30:70] = S.random_plane(rng, 40, 20, obstacles=0.3)
    shifted = S.random_plane(rng, w, h, obstacles=0.12)
    goals = fields_of(rng, w, h, plane)[:7]
    dev = lom.NavFieldSet(RES, ORIGIN, w, h, 7)
    summaries = dev.solve(plane, as_tuple(P1), goals)
    kept = [dev.potential(i) for i in range(7)]
    starts = np.concatenate([np.stack([rng.integers(0, w, 30), rng.integers(0, h, 30)], axis=1), [(0, 0), (-1, 4), (w, h)]]).astype(np.int32)
    xy = (np.array(ORIGIN) + rng.uniform(-2, max(w, h) + 2, (60, 2)) * RES).astype(np.float32)
    wp = (0, 12, 200, 0)
    for i in (0, 1, 2, 5, 6):
        adopted, direct = lom.NavField(RES, ORIGIN, w, h), lom.NavField(RES, ORIGIN, w, h)
        if i == 5:                                    # over a field that holds something else, and a second block
            adopted.solve(shifted, as_tuple(P0), goals[0])
            adopted.shiftResolve(3, 3, shifted)
            adopted.shift(-3, -3)
        assert direct.solve(plane, as_tuple(P1), goals[i]) == summaries[i]
        assert adopted.adopt(dev, i) == summaries[i]
        assert adopted.geometry() == direct.geometry()
        assert adopted.potential().tobytes() == direct.potential().tobytes() == dev.potential(i).tobytes()
        for a, b in zip(adopted.paths(starts, 50), direct.paths(starts, 50)):
            assert a.tobytes() == b.tobytes()
        for a, b in zip(adopted.waypoints(starts, wp, 20), direct.waypoints(starts, wp, 20)):
            assert a.tobytes() == b.tobytes()
        assert adopted.query(xy).tobytes() == direct.query(xy).tobytes()
        pairs = np.concatenate([starts[:20], starts[10:30]], axis=1)
        assert adopted.visible(pairs).tobytes() == direct.visible(pairs).tobytes()
        # a re-solve with a changed window, then a shift with a re-solve
        window = (25, 15, 50, 30)
        assert adopted.resolve(changed, window) == direct.resolve(changed, window)
        assert adopted.potential().tobytes() == direct.potential().tobytes()
        assert adopted.resolveStats()["cells_changed"] == direct.resolveStats()["cells_changed"] > 0
        assert adopted.shiftResolve(7, -4, shifted) == direct.shiftResolve(7, -4, shifted)
        assert adopted.potential().tobytes() == direct.potential().tobytes() and adopted.geometry() == direct.geometry()
        assert adopted.shiftStats() == direct.shiftStats()
        assert dev.potential(i).tobytes() == kept[i].tobytes()                  # the set goes on: its field is untouched
    assert dev.fieldCount() == 7


def test_refused_adopts_leave_the_field(lom):
    w, h = 33, 31
    plane = S.pocket(w, h)
    L = lom.capi.lib()
    dev = lom.NavFieldSet(RES, ORIGIN, w, h, 3)
    field = lom.NavField(RES, ORIGIN, w, h)
    want = field.solve(plane, as_tuple(P0), np.array([(0, 0)], np.int32))
    before = field.potential()

    def refused(code, fieldset, i):
        sm = lom.capi.NavFieldSummary(*([9] * 8))
        assert L.lom_navfield_adopt(field.handle, fieldset.handle if fieldset is not None else None, i, C.byref(sm)) == code
        assert sm.asdict() == dict.fromkeys(N.SUMMARY_KEYS, 0)
        assert field.potential().tobytes() == before.tobytes()
        assert field.resolve(plane, (0, 0, 0, 0)) == want                      # still solved, with its own summary words

    refused(lom.capi.ERR_STATE, dev, 0)                                             # a set with no solve
    dev.solve(np.zeros((h, w), np.int8), as_tuple(P0), [np.array([(5, 5)], np.int32), np.zeros((0, 2), np.int32)])
    refused(lom.capi.ERR_ARG, dev, 2)                                               # i out of range
    refused(lom.capi.ERR_ARG, dev, 2 ** 40)
    refused(lom.capi.ERR_ARG, None, 0)
    other = lom.NavFieldSet(RES, (ORIGIN[0], -ORIGIN[1]), w, h, 1)
    other.solve(plane, as_tuple(P0), [np.array([(1, 1)], np.int32)])
    refused(lom.capi.ERR_ARG, other, 0)                                             # a geometry that is not bit-equal
    wider = lom.NavFieldSet(RES, ORIGIN, w + 1, h, 1)
    wider.solve(np.zeros((h, w + 1), np.int8), as_tuple(P0), [np.array([(1, 1)], np.int32)])
    refused(lom.capi.ERR_ARG, wider, 0)
    dev.clear()
    refused(lom.capi.ERR_STATE, dev, 0)
    dev.solve(np.zeros((h, w), np.int8), as_tuple(P0), [np.array([(5, 5)], np.int32)])
    dev.shift(1, 0)
    refused(lom.capi.ERR_ARG, dev, 0)                                               # shifted: another geometry
    dev.shift(-1, 0)
    refused(lom.capi.ERR_STATE, dev, 0)                                             # ... and no solve since
    # and an adopt that is not refused works behind all of them
    dev.solve(np.zeros((h, w), np.int8), as_tuple(P0), [np.array([(5, 5)], np.int32)])
    assert field.adopt(dev, 0)["goals_used"] == 1 and field.potential()[5, 5] == 0


# ---- 6: the forms of a solve -------------------------------------------------------------------------------------------------
def clearance_case(lom):
    """a clearance grid with its cost plane, six goal lists on it and their references"""
    rng = np.random.default_rng(19)
    w, h = 90, 47
    occ = np.where(rng.random((h, w)) < 0.01, 100, 0).astype(np.int8)
    occ[rng.random((h, w)) < 0.02] = -1
    clear = lom.ClearanceGrid(RES, ORIGIN, w, h)
    clear.update(occ, None, K.params(1.0, 0.3, 1.5))
    cost = clear.cost()[0]
    goals = fields_of(rng, w, h, cost)[:6]
    return w, h, clear, cost, goals, references("forms", w, h, cost, P1, goals)


def test_solve_from_clearance_equals_solve(lom):
    w, h, clear, cost, goals, refs = clearance_case(lom)
    host, dev = lom.NavFieldSet(RES, ORIGIN, w, h, 6), lom.NavFieldSet(RES, ORIGIN, w, h, 6)
    want = host.solve(cost, as_tuple(P1), goals)
    assert dev.solveFromClearance(clear, as_tuple(P1), goals) == want
    for i in range(6):
        assert host.potential(i).tobytes() == dev.potential(i).tobytes() == refs[i]["P"].tobytes() and want[i] == refs[i]["summary"]
    assert np.array_equal(clear.cost()[0], cost)                                    # the producer goes on
    clear.update(np.zeros((h, w), np.int8), None, K.params(1.0, 0.3, 1.5))
    assert dev.potential(3).tobytes() == refs[3]["P"].tobytes()                     # the set keeps its own copy of the plane
    # a clearance grid of another geometry: refused, nothing changes
    for bad in (lom.ClearanceGrid(RES, ORIGIN, w + 1, h), lom.ClearanceGrid(RES, (ORIGIN[0] + 1e-6, ORIGIN[1]), w, h)):
        with pytest.raises(lom.LomError) as e:
            dev.solveFromClearance(bad, as_tuple(P1), goals[:2])
        assert e.value.code == lom.capi.ERR_ARG and dev.fieldCount() == 6
        assert dev.potential(5).tobytes() == refs[5]["P"].tobytes()


def test_solve_device_behind_an_event_equals_solve(lom):
    import torch

    w, h, clear, cost, goals, refs = clearance_case(lom)
    late = lom.NavFieldSet(RES, ORIGIN, w, h, 6)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        big = torch.ones(1 << 22, device="cuda:0")
        for _ in range(10):                                                       # work in front of the plane
            big = big * 1.0001 + 1.0
        t_cost = torch.from_numpy(cost).to("cuda:0", non_blocking=True) + 0
        ev = torch.cuda.Event()
        ev.record(stream)
    got = late.solveDevice(t_cost.data_ptr(), as_tuple(P1), goals, hip_event=C.c_void_p(ev.cuda_event))
    torch.cuda.synchronize()
    for i in range(6):
        assert late.potential(i).tobytes() == refs[i]["P"].tobytes() and got[i] == refs[i]["summary"]
    # ... and with no event, the clearance grid's own plane in HBM, complete since update() returned
    d_cost = C.c_void_p()
    assert lom.capi.lib().lom_clearance_cost_device(clear.handle, C.byref(d_cost)) == 0
    assert late.solveDevice(d_cost.value, as_tuple(P1), goals[::-1]) == [r["summary"] for r in refs[::-1]]
    assert late.potential(0).tobytes() == refs[5]["P"].tobytes()


def test_the_chain_to_the_rollouts(lom):
    """ClearanceGrid -> NavFieldSet -> adopt -> RolloutGrid.evaluateFromGrids equals the references' chain"""
    table = lom.visibilityTable(R.TABLE)
    rng = np.random.default_rng(21)
    w, h = 90, 47
    geo = K.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)
    occ = np.where(rng.random((h, w)) < 0.01, 100, 0).astype(np.int8)
    occ[rng.random((h, w)) < 0.02] = -1
    cp = K.params(1.0, 0.3, 1.5)
    nav_params = (50, 3, 400, 98, 1)
    goals = [np.array([[3, 3]], np.int32), np.array([[w - 5, h // 2], [3, 3]], np.int32), np.array([[w // 2, h - 2]], np.int32)]
    clear, navs, nav = lom.ClearanceGrid(RES, ORIGIN, w, h), lom.NavFieldSet(RES, ORIGIN, w, h, 3), lom.NavField(RES, ORIGIN, w, h)
    clear.update(occ, None, cp)
    navs.solveFromClearance(clear, nav_params, goals)
    cost = K.update(geo, occ, None, cp, table=lom.clearanceCostTable(cp, RES))["cost"]
    assert np.array_equal(clear.cost()[0], cost)
    fp = lom.rolloutFootprintRectangle(300, 200, 150, 100, True)
    states, cmd = states_of(cost, rng, 6), commands_of(rng, 200, 2)
    p = R.params(2, 40, 99, 30, min_steps=10, progress_weight=4, cost_weight=1, truncation_weight=100)
    dev = lom.RolloutGrid(RES, ORIGIN, w, h)
    for i in (1, 2):
        potential = N.solve(N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h), cost, N.params(*nav_params), goals[i])["P"]
        nav.adopt(navs, i)
        assert np.array_equal(nav.potential(), potential) and (potential != R.UNREACHED).sum() > 1000
        ref = R.evaluate_fast(cost, potential, states, cmd, fp, table, p)
        assert ref["summary"]["admissible"] > 100
        picks, summary = dev.evaluateFromGrids(clear, nav, states, cmd, fp, R.as_tuple(p))
        assert summary == ref["summary"] and picks.tobytes() == ref["picks"].tobytes() and dev.records().tobytes() == ref["records"].tobytes()
    assert np.array_equal(clear.cost()[0], cost) and navs.fieldCount() == 3           # the producers go on


# ---- 7: the state of a set ---------------------------------------------------------------------------------------------------
def test_fewer_fields_after_more_twice_the_same_and_max_fields_of_one(lom):
    w, h = 65, 33
    rng = np.random.default_rng(23)
    plane = S.random_plane(rng, w, h, obstacles=0.15)
    goals = fields_of(rng, w, h, plane)[:9]
    refs = references("state", w, h, plane, P0, goals)
    dev = lom.NavFieldSet(RES, ORIGIN, w, h, 9)
    assert dev.fieldCount() == 0 and dev.stats() == dict(launches=0, waits=0, tiles=0, fields=0)
    check_set(dev, refs, plane, P0, goals)
    first = [dev.potential(i) for i in range(9)]
    # fewer fields, other goals: the count and the bytes of the smaller
    fewer = [goals[8], goals[3]]
    check_set(dev, [refs[8], refs[3]], plane, P0, fewer)
    assert dev.fieldCount() == 2
    with pytest.raises(lom.LomError) as e:
        dev.potential(2)
    assert e.value.code == lom.capi.ERR_ARG
    assert dev.gather(np.array([(1, 1)], np.int32)).shape == (2, 1)
    # twice the same
    check_set(dev, refs, plane, P0, goals)
    assert all(dev.potential(i).tobytes() == first[i].tobytes() for i in range(9))
    # none at all
    assert dev.solve(plane, as_tuple(P0), []) == [] and dev.fieldCount() == 0 and dev.stats()["launches"] == 0
    # a set of one
    one = lom.NavFieldSet(RES, ORIGIN, w, h, 1)
    check_set(one, refs[:1], plane, P0, goals[:1])
    owner, potential, owned = one.nearest()
    assert potential.tobytes() == refs[0]["P"].tobytes() and int(owned[0]) == refs[0]["summary"]["cells_reached"]
    with pytest.raises(lom.LomError) as e:
        one.solve(plane, as_tuple(P0), goals[:2])
    assert e.value.code == lom.capi.ERR_ARG and one.fieldCount() == 1
    for bad in (0, 65536, -1):
        with pytest.raises((lom.LomError, OverflowError, ValueError)):
            lom.NavFieldSet(RES, ORIGIN, w, h, bad)


def test_shift_equals_a_fresh_cleared_set(lom):
    from tests import grid_shift_ref as GS

    w, h = 65, 33
    rng = np.random.default_rng(29)
    plane, moved_plane = S.random_plane(rng, w, h, obstacles=0.1), S.random_plane(rng, w, h, obstacles=0.1)
    goals = fields_of(rng, w, h, plane)[:4]
    dev = lom.NavFieldSet(RES, ORIGIN, w, h, 4)
    dev.solve(plane, as_tuple(P0), goals)
    dev.shift(5, -3)
    moved = GS.shift_geometry(geo_of(w, h), 5, -3)[1]
    assert GS.geometry_bits(dev.geometry()) == GS.geometry_bits(moved)
    assert dev.fieldCount() == 0 and dev.stats() == dict(launches=0, waits=0, tiles=0, fields=0)
    with pytest.raises(lom.LomError) as e:
        dev.nearest()
    assert e.value.code == lom.capi.ERR_STATE
    fresh = lom.NavFieldSet(float(moved["resolution"]), (float(moved["origin_x"]), float(moved["origin_y"])), w, h, 4)
    assert GS.geometry_bits(fresh.geometry()) == GS.geometry_bits(moved)
    # ... and solves as the fresh one does, goals in metres landing in the moved cells
    xy = [(np.array([moved["origin_x"], moved["origin_y"]], np.float64) + (g + 0.5) * RES).astype(np.float32) for g in goals]
    assert dev.solve(moved_plane, as_tuple(P0), xy, metres=True) == fresh.solve(moved_plane, as_tuple(P0), xy, metres=True)
    assert all(dev.potential(i).tobytes() == fresh.potential(i).tobytes() for i in range(4))
    assert dev.potential(0).tobytes() == N.solve(moved, moved_plane, P0, xy[0], True)["P"].tobytes()
    # a shift the rule refuses (the origin would not be finite) leaves the set
    far = lom.NavFieldSet(1e30, (3e38, 0.0), w, h, 2)
    far.solve(plane, as_tuple(P0), [np.array([(1, 1)], np.int32), np.array([(w - 1, 0)], np.int32)])
    before, geo_before = [far.potential(i) for i in range(2)], far.geometry()
    with pytest.raises(lom.LomError) as e:
        far.shift(2 ** 31 - 1, 0)
    assert e.value.code == lom.capi.ERR_RANGE and far.fieldCount() == 2 and far.geometry() == geo_before
    assert all(far.potential(i).tobytes() == before[i].tobytes() for i in range(2))


def test_every_refusal_changes_nothing(lom):
    w, h = 33, 31
    L = lom.capi.lib()
    rng = np.random.default_rng(31)
    plane = S.random_plane(rng, w, h, obstacles=0.1)
    goals = fields_of(rng, w, h, plane)[:3]
    dev = lom.NavFieldSet(RES, ORIGIN, w, h, 4)
    dev.solve(plane, as_tuple(P0), goals)
    before, stats = [dev.potential(i) for i in range(3)], dev.stats()
    all_goals, offsets = NS.offsets_of(goals)
    all_goals = np.ascontiguousarray(all_goals, np.int32)
    other = np.zeros((h, w), np.int8)
    good = lom.navfieldParams(as_tuple(P0))

    def refused(plane_ptr, params, kind, goals_ptr, offsets_arr, n_fields, form="solve"):
        sm = (lom.capi.NavFieldSummary * 5)(*[lom.capi.NavFieldSummary(*([9] * 8)) for _ in range(5)])
        keep = None if offsets_arr is None else np.array(offsets_arr, np.uint32)            # (alive across the call)
        off_ptr = None if keep is None else keep.ctypes.data
        if form == "solve":
            rc = L.lom_navset_solve(dev.handle, plane_ptr, params, kind, goals_ptr, off_ptr, n_fields, sm)
        else:
            rc = L.lom_navset_solve_device(dev.handle, plane_ptr, None, params, kind, goals_ptr, off_ptr, n_fields, sm)
        assert rc == lom.capi.ERR_ARG, rc
        zeroed = min(n_fields, 4)
        assert all(sm[i].asdict() == dict.fromkeys(N.SUMMARY_KEYS, 0) for i in range(zeroed))
        assert all(sm[i].cells_blocked == 9 for i in range(zeroed, 5))
        assert dev.fieldCount() == 3 and dev.stats() == stats
        assert all(dev.potential(i).tobytes() == before[i].tobytes() for i in range(3))

    g, o, p = all_goals.ctypes.data, offsets, C.byref(good)
    for form in ("solve", "device"):
        refused(None, p, 0, g, o, 3, form)                                                    # no plane
        refused(other.ctypes.data, None, 0, g, o, 3, form)                                    # no parameters
        refused(other.ctypes.data, C.byref(lom.navfieldParams((0, 3, 400, 98, 0))), 0, g, o, 3, form)
        refused(other.ctypes.data, p, 2, g, o, 3, form)                                       # an unknown goal kind
        refused(other.ctypes.data, p, 0, g, list(o) + [o[-1]] * 2, 5, form)                   # more fields than the set holds
        refused(other.ctypes.data, p, 0, g, None, 3, form)                                    # no offsets
        refused(other.ctypes.data, p, 0, g, [1] + list(o[1:]), 3, form)                       # a start that is not 0
        refused(other.ctypes.data, p, 0, g, [0, 5, 4, int(o[-1])], 3, form)                   # falling
        refused(other.ctypes.data, p, 0, g, [0, 1, 2, (1 << 24) + 1], 3, form)                # too many goals
        refused(other.ctypes.data, p, 0, None, o, 3, form)                                    # goals missing
    # gather and potential
    out = np.full((3, 2), 7, np.uint32)
    pts = np.array([(0, 0), (1, 1)], np.int32)
    assert L.lom_navset_gather(dev.handle, 5, pts.ctypes.data, 2, out.ctypes.data) == lom.capi.ERR_ARG
    assert L.lom_navset_gather(dev.handle, 0, None, 2, out.ctypes.data) == lom.capi.ERR_ARG
    assert L.lom_navset_gather(dev.handle, 0, pts.ctypes.data, 2, None) == lom.capi.ERR_ARG
    assert L.lom_navset_gather(dev.handle, 0, pts.ctypes.data, (1 << 24) + 1, out.ctypes.data) == lom.capi.ERR_ARG
    assert L.lom_navset_gather(dev.handle, 0, pts.ctypes.data, 1 << 27, out.ctypes.data) == lom.capi.ERR_ARG
    assert (out == 7).all()
    assert L.lom_navset_potential(dev.handle, 3, out.ctypes.data, 2) == lom.capi.ERR_ARG and (out == 7).all()
    ptr = C.c_void_p(5)
    assert L.lom_navset_potential_device(dev.handle, 3, C.byref(ptr)) == lom.capi.ERR_ARG and not ptr.value
    assert L.lom_navset_potential_device(dev.handle, 2, C.byref(ptr)) == 0 and ptr.value == dev.potentialDevice(0) + 2 * w * h * 4
    for option, bad in ((lom.capi.NAVSET_OPT_TEST_INNER_CAP, (1 << 20) + 1), (lom.capi.NAVSET_OPT_TEST_BATCH, 257),
                        (lom.capi.NAVSET_OPT_TEST_ALL_TILES, 2), (99, 0)):
        with pytest.raises(lom.LomError) as e:
            dev.setOption(option, bad)
        assert e.value.code == lom.capi.ERR_ARG
    assert dev.fieldCount() == 3 and all(dev.potential(i).tobytes() == before[i].tobytes() for i in range(3))
    # and the set still solves
    check_set(dev, references("refusals", w, h, plane, P0, goals), plane, P0, goals)


# ---- 8: the C++ mirror -------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::NavFieldSet and lom::NavField::adopt of the C++ mirror compile with plain g++ and leave the bytes the reference gives"""
    exe = cpp_program.build_with_library(tmp_path, "test_navset_mirror.cpp")
    stdout = cpp_program.run(exe, "device", timeout=120)
    lines = stdout.strip().split("\n")
    # the same grid, plane and goals here (tests/cpp/test_navset_mirror.cpp)
    w, h = 45, 37
    i = np.arange(w * h)
    plane = np.where(i % 7 == 3, 100, np.where(i % 5 == 0, -1, (i % 13) * 7)).astype(np.int8).reshape(h, w)
    goals = [np.array([(0, 0), (44, 36)], np.int32), np.array([(21, 20)], np.int32), np.array([(44, 36), (-1, 5)], np.int32)]
    p = N.params(20, 2, 300, 80, N.UNKNOWN_PASSABLE)
    refs = NS.solve_set(geo_of(w, h), plane, p, goals)
    for k, ref in enumerate(refs):
        assert [int(v) for v in lines[-8 + k].split()] == [ref["summary"][key] for key in N.SUMMARY_KEYS], k
        got = np.array([int(v) for v in lines[-3 + k].split()], np.uint64).astype(np.uint32)
        assert got.tobytes() == ref["P"].tobytes(), k
    at = np.array([(0, 0), (21, 20), (44, 36)], np.int32)
    assert [int(v) for v in lines[-5].split()] == NS.gather(geo_of(w, h), refs, at).reshape(-1).tolist()
    assert [int(v) for v in lines[-4].split()] == NS.nearest(geo_of(w, h), refs)[2].tolist()
