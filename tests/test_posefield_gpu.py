"""The pose field on the device against tests/posefield_ref.py: the layers, the field, the floor with its headings, the
summary, the paths with their lengths and the query -- all as bytes, with no tolerance, under every setting of the three
test switches.  The reference of a case is computed once and shared.  Goals are drawn from the states the reference calls
passable, and the tests that are about coverage assert on the reference, before they look at the device, that a case
reaches at least half of the passable states."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import navfield_ref as N
from tests import posefield_ref as R
from tests import posefield_scenes as S
from tests import rollout_ref as X

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)
NAV = N.params(50, 3, 400, 98)
NAV_UNKNOWN = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)
BOTH = R.SPIN | R.REVERSE
P_BOTH = R.params(NAV, 20, 1, 200, BOTH)
TILE = (32, 8)
# the navigation field's seven shapes, and one cell less than, exactly and one cell more than a tile on each axis
SHAPES = [(1, 1), (1, 70), (70, 1), (32, 32), (33, 31), (65, 33), (129, 65),
          (TILE[0] - 1, TILE[1] - 1), (TILE[0], TILE[1]), (TILE[0] + 1, TILE[1] + 1), (TILE[0] - 1, TILE[1] + 1), (TILE[0] + 1, TILE[1] - 1)]
# inner cap (0: the default), batch, all tiles
SWITCHES = [(cap, batch, every) for cap in (1, 0) for batch in (1, 8) for every in (0, 1)]
FOOTPRINTS = {"point": S.POINT, "5x3": S.RECT_5x3, "9x3": S.RECT_9x3, "L": S.L_SHAPE, "1024": S.big(np.random.default_rng(3))}
# flags x turn_cost x spin_cost x reverse_cost
PARAM_SETS = [R.params(NAV, turn, spin, rev, flags) for flags in (0, R.SPIN, R.REVERSE, BOTH) for turn in (0, 20)
              for spin in (1, R.MAX_COST) for rev in (0, 200)]
REFS = {}


def geo_of(w, h):
    return N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)


def reference(key, w, h, plane, p, fp, goals):
    """the reference's solve of a case, once"""
    if key not in REFS:
        REFS[key] = R.solve(geo_of(w, h), plane, p, fp, goals)
    return REFS[key]


def set_switches(lom, dev, cap, batch, every):
    dev.setOption(lom.capi.POSE_OPT_TEST_INNER_CAP, cap)
    dev.setOption(lom.capi.POSE_OPT_TEST_BATCH, batch)
    dev.setOption(lom.capi.POSE_OPT_TEST_ALL_TILES, every)


def check_field(dev, ref, what):
    """what a solve left against the reference: layers, field, floor, floor heading"""
    got = dev.layers()
    assert got.tobytes() == ref["L"].tobytes(), (what, "layers", np.argwhere(got != ref["L"])[:10])
    got = dev.potential()
    assert got.tobytes() == ref["P"].tobytes(), (what, "field", np.argwhere(got != ref["P"])[:10])
    fl, fh = dev.floor()
    assert fl.tobytes() == ref["floor"].tobytes(), (what, "floor")
    assert fh.tobytes() == ref["floor_heading"].tobytes(), (what, "floor heading")


def check_solve(dev, ref, plane, p, fp, goals, what=None):
    summary = dev.solve(plane, R.as_tuple(p), fp, goals)
    assert not ref["error"] and summary == ref["summary"], (what, summary, ref["summary"])
    check_field(dev, ref, what)
    st = dev.stats()
    assert st["launches"] >= 1 and 1 <= st["waits"] <= st["launches"]


def some_starts(rng, ref, w, h, n):
    """reached states, cells under h = -1 all over the grid, and starts that are not walked"""
    s = [(int(rng.integers(0, w)), int(rng.integers(0, h)), -1) for _ in range(n)]
    reached = np.argwhere(ref["P"] != R.UNREACHED)
    if len(reached):
        s += [(int(x), int(y), int(hd)) for hd, y, x in reached[rng.choice(len(reached), min(n, len(reached)), replace=False)]]
        far = reached[np.argmax(ref["P"][tuple(reached.T)])]
        s.append((int(far[2]), int(far[1]), int(far[0])))
    s += [(0, 0, -1), (w - 1, h - 1, 3), (-1, 0, 0), (w, h - 1, -1), (0, h, 2), (0, 0, 8), (0, 0, -2)]
    return np.array(s, np.int32)


def check_paths_and_query(dev, ref, p, rng, w, h, what, cap=40):
    starts = some_starts(rng, ref, w, h, 5)
    states, lengths = dev.paths(starts, cap)
    want_states, want_lengths = R.paths(ref, p, starts, cap)
    assert np.array_equal(lengths, want_lengths), (what, lengths, want_lengths)
    assert states.tobytes() == want_states.tobytes(), what
    xy = np.concatenate([rng.uniform(ORIGIN[0] - 1.0, ORIGIN[0] + w * RES + 1.0, (60, 1)),
                         rng.uniform(ORIGIN[1] - 1.0, ORIGIN[1] + h * RES + 1.0, (60, 1))], axis=1).astype(np.float32)
    xy[0] = (np.nan, 3.0)
    hd = rng.integers(-2, 10, 60).astype(np.int32)
    assert np.array_equal(dev.query(xy, hd), R.query(geo_of(w, h), ref, xy, hd)), what


def passable_goals(rng, L, n, any_heading_every=3):
    """n goals drawn from the passable states; every third names its cell under h = -1"""
    states = np.argwhere(L != 0)
    if not len(states):
        return np.zeros((0, 3), np.int32)
    pick = states[rng.choice(len(states), min(n, len(states)), replace=False)]
    return np.array([(x, y, -1 if k % any_heading_every == 0 else hd) for k, (hd, y, x) in enumerate(pick.tolist())], np.int32)


def layers_of(plane, p, fp):
    return R.layers(plane, p, R.stencils(fp))


def scenes_of(w, h):
    """name -> (plane, nav parameters)"""
    rng = np.random.default_rng(1000 * w + h)
    out = {
        "empty": (S.empty(w, h), NAV),
        "sparse2": (S.sparse(rng, w, h, 0.02), NAV),
        "sparse5": (S.sparse(rng, w, h, 0.05), NAV),
        "serpentine": (S.serpentine(w, h), NAV),
        "spiral": (S.spiral(w, h), NAV),
        "diagonal_gaps": (S.diagonal_gaps(w, h), NAV),
        "pocket": (S.pocket(w, h), NAV),
        "all_blocked": (S.all_blocked(w, h), NAV),
        "unknown": (np.where(rng.random((h, w)) < 0.1, -1, S.sparse(rng, w, h, 0.02)).astype(np.int8), NAV_UNKNOWN),
        "invalid_bytes": (S.with_unknown_and_invalid(rng, w, h), NAV),
    }
    if w >= 30 and h >= 30:
        out["l_corridor5"] = (S.l_corridor(w, h, 5)[0], NAV)
        out["l_corridor9"] = (S.l_corridor(w, h, 9)[0], NAV)
        out["doorway"] = (S.doorway(w, h)[0], NAV)
    return out


# ---- 1: shapes x scenes x switches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_scenes_and_switches(lom, w, h):
    rng = np.random.default_rng(w + 7 * h)
    dev = lom.PoseField(RES, ORIGIN, w, h)
    names = list(FOOTPRINTS)
    scenes = scenes_of(w, h)
    if (w, h) == (129, 65):                                          # the largest shape: the scenes with the longest routes
        scenes = {k: scenes[k] for k in ("empty", "sparse2", "serpentine", "spiral", "invalid_bytes")}
    for k, (name, (plane, nav)) in enumerate(scenes.items()):
        # The one-cell corridors take a point that spins at a low cost (a corner cannot be rounded by FL or FR: the
        # diagonal step between is cut off) and one far goal; the other scenes rotate through the footprints and the
        # parameter sets, with goals drawn from the passable states.
        corridors = name in ("serpentine", "spiral")
        fp_name = "point" if corridors else names[(k + w) % len(names)]
        which = (8 if (w + h) % 2 else 24) + (0, 1, 4, 5)[(k + w) % 4] if corridors else (5 * k + w + h) % len(PARAM_SETS)
        p = dict(PARAM_SETS[which], nav=nav)
        fp = FOOTPRINTS[fp_name]
        goals = np.array([(0, 0, -1)], np.int32) if corridors else passable_goals(rng, layers_of(plane, p, fp), 4)
        goals = np.concatenate([goals, np.array([(-1, 0, 0), (0, 0, 8)], np.int32)])
        ref = reference((w, h, name), w, h, plane, p, fp, goals)
        for cap, batch, every in SWITCHES:
            set_switches(lom, dev, cap, batch, every)
            check_solve(dev, ref, plane, p, fp, goals, what=(name, fp_name, cap, batch, every))
        check_paths_and_query(dev, ref, p, rng, w, h, name)
        assert ref["summary"]["goals_rejected"] >= 2
    if (w, h) == (129, 65):
        # what the scenes are for, on the reference; and the default switches take fewer launches than one sweep per launch
        assert REFS[(w, h, "serpentine")]["summary"]["states_reached"] > 4000
        assert REFS[(w, h, "spiral")]["summary"]["max_potential"] > 250 * 2000
        plane, nav = scenes["serpentine"]
        p, goals = dict(P_BOTH, nav=nav), np.array([(0, 0, -1)], np.int32)
        set_switches(lom, dev, 1, 8, 1)
        dev.solve(plane, R.as_tuple(p), S.POINT, goals)
        slow = dev.stats()["launches"]
        set_switches(lom, dev, 0, 0, 0)
        dev.solve(plane, R.as_tuple(p), S.POINT, goals)
        assert dev.stats()["launches"] < slow


# ---- 2: every scene under every footprint, with at least half of the passable states reached ---------------------------------------
@pytest.mark.parametrize("fp_name", list(FOOTPRINTS))
def test_every_scene_under_every_footprint(lom, fp_name):
    w, h = 65, 33
    rng = np.random.default_rng(len(fp_name) + 11)
    fp = FOOTPRINTS[fp_name]
    dev = lom.PoseField(RES, ORIGIN, w, h)
    for name, (plane, nav) in scenes_of(w, h).items():
        p = dict(P_BOTH, nav=nav)
        L = layers_of(plane, p, fp)
        # many goals all over the passable states: with spins and the reverse they reach most of what is passable
        goals = passable_goals(rng, L, 24, any_heading_every=2)
        ref = reference(("cover", fp_name, name), w, h, plane, p, fp, goals)
        sm = ref["summary"]
        passable = sm["states_reached"] + sm["states_unreached"]
        if name != "all_blocked":
            # on the reference, before the device is looked at.  (A footprint wider than a one-cell corridor has no passable
            # state there; then there is nothing to reach.)
            assert 2 * sm["states_reached"] >= passable and (sm["states_reached"] > 0 or passable == 0), (name, sm)
        else:
            assert passable == 0 and sm["states_reached"] == 0
        for cap, batch, every in ((0, 0, 0), (1, 1, 0)):
            set_switches(lom, dev, cap, batch, every)
            check_solve(dev, ref, plane, p, fp, goals, what=(name, fp_name, cap))
        check_paths_and_query(dev, ref, p, rng, w, h, (name, fp_name))
    # the centre goal under h = -1 on 2 % obstacles: the 5 x 3 rectangle reaches most of the grid under every flag set
    if fp_name == "5x3":
        plane, nav = scenes_of(w, h)["sparse2"]
        L = layers_of(plane, P_BOTH, fp)
        centre = np.argwhere(L.any(axis=0))
        cy, cx = centre[np.argmin(np.abs(centre - (h // 2, w // 2)).sum(axis=1))]
        goals = np.array([(cx, cy, -1)], np.int32)
        for flags in (0, R.SPIN, R.REVERSE, BOTH):
            p = R.params(nav, 20, 2, 200, flags)
            ref = reference(("centre", flags), w, h, plane, p, fp, goals)
            sm = ref["summary"]
            assert 2 * sm["states_reached"] >= sm["states_reached"] + sm["states_unreached"], (flags, sm)
            check_solve(dev, ref, plane, p, fp, goals, what=("centre", flags))


# ---- 3: parameter sets -----------------------------------------------------------------------------------------------------------
def test_parameter_sets(lom):
    w, h = 33, 31
    rng = np.random.default_rng(8)
    plane, nav = scenes_of(w, h)["sparse2"]
    fp = S.RECT_5x3
    goals = passable_goals(rng, layers_of(plane, P_BOTH, fp), 3)
    dev = lom.PoseField(RES, ORIGIN, w, h)
    seen = set()
    for k, p in enumerate(PARAM_SETS):
        ref = reference(("params", k), w, h, plane, p, fp, goals)
        check_solve(dev, ref, plane, p, fp, goals, what=("params", k))
        check_paths_and_query(dev, ref, p, rng, w, h, ("params", k), cap=12)
        seen.add(ref["P"].tobytes())
    assert len(seen) >= 12                                           # the parameters matter


def test_range_exceeded_and_dropped_candidates(lom):
    """cells of the greatest cost on the serpentine: the route's weight passes LOM_NAV_MAX, candidates are dropped and the
    states behind them stay unreached"""
    w, h = 65, 33
    plane = S.serpentine(w, h)
    p = R.params(N.params(R.MAX_COST, 0, 1, 98), R.MAX_COST, R.MAX_COST, R.MAX_COST, BOTH)
    goals = np.array([(0, 0, -1)], np.int32)
    ref = reference("range", w, h, plane, p, S.POINT, goals)
    sm = ref["summary"]
    assert sm["range_exceeded"] == 1 and sm["states_unreached"] > 0 and sm["states_reached"] > 100
    assert sm["max_potential"] > R.MAX - 8 * R.MAX_COST
    dev = lom.PoseField(RES, ORIGIN, w, h)
    for cap, batch, every in SWITCHES[::3]:
        set_switches(lom, dev, cap, batch, every)
        check_solve(dev, ref, plane, p, S.POINT, goals, what=("range", cap, batch, every))
    check_paths_and_query(dev, ref, p, np.random.default_rng(1), w, h, "range")
    # the same costs on a corridor of 41 cells: 41 * 5 * 2^24 and four spins stay below LOM_NAV_MAX, and nothing is exceeded
    small = reference("range_not", 20, 3, S.serpentine(20, 3), p, S.POINT, goals)
    assert small["summary"]["range_exceeded"] == 0 and small["summary"]["states_unreached"] == 0
    assert small["summary"]["max_potential"] > 1 << 31
    low = lom.PoseField(RES, ORIGIN, 20, 3)
    check_solve(low, small, S.serpentine(20, 3), p, S.POINT, goals, what="range_not")


# ---- 4: goal sets ----------------------------------------------------------------------------------------------------------------
def test_degenerate_goal_sets(lom):
    w, h = 33, 31
    plane, (door_x, door_y) = S.doorway(w, h)
    fp, p = S.RECT_9x3, P_BOTH
    L = layers_of(plane, p, fp)
    assert L[:, door_y, door_x].astype(bool).tolist() == [True, False, False, False, True, False, False, False]
    blocked_cell = (door_x, door_y + 5)                              # in the wall: no passable heading
    assert not L[:, blocked_cell[1], blocked_cell[0]].any() and not L[:, 0, 0].any()   # ... and a corner never fits a 9 x 3
    free = (6, h // 2)
    assert L[:, free[1], free[0]].all()
    border = [(x, y, -1) for x in (0, 4, w - 5, w - 1) for y in (0, 4, h - 5, h - 1)]
    sets = {
        "none": np.zeros((0, 3), np.int32),
        "only rejected": [(-1, 0, 0), (w, 0, -1), (0, h, 3), (3, 3, 8), (3, 3, -2), blocked_cell + (-1,), (door_x, door_y, 2),
                          (-(2 ** 31), 2 ** 31 - 1, 0)],
        "no passable heading": [blocked_cell + (-1,), (0, 0, -1)],
        "duplicates": [free + (2,), free + (2,), free + (2,)],
        "two headings of a cell": [free + (0,), free + (5,), free + (-1,), free + (0,)],
        "border cells": border,
        "the doorway itself": [(door_x, door_y, -1)],
    }
    want_used = {"none": 0, "only rejected": 0, "no passable heading": 0, "duplicates": 1, "two headings of a cell": 8,
                 "the doorway itself": 2}
    dev = lom.PoseField(RES, ORIGIN, w, h)
    for name, goals in sets.items():
        goals = np.array(goals, np.int32).reshape(-1, 3)
        ref = reference(("goals", name), w, h, plane, p, fp, goals)
        if name in want_used:
            assert ref["summary"]["goals_used"] == want_used[name], name
        if name in ("only rejected", "no passable heading"):
            assert ref["summary"]["goals_rejected"] == len(goals) and ref["summary"]["states_reached"] == 0
        for cap, batch, every in SWITCHES[::3]:
            set_switches(lom, dev, cap, batch, every)
            check_solve(dev, ref, plane, p, fp, goals, what=("goals", name, cap, batch, every))
        check_paths_and_query(dev, ref, p, np.random.default_rng(4), w, h, ("goals", name))
    assert REFS[("goals", "border cells")]["summary"]["goals_rejected"] >= 4      # the corners
    assert REFS[("goals", "the doorway itself")]["summary"]["states_reached"] > 1000


# ---- 5: the other families ---------------------------------------------------------------------------------------------------------
def test_point_footprint_against_the_navigation_field(lom):
    w, h = 65, 33
    rng = np.random.default_rng(31)
    plane = S.with_unknown_and_invalid(rng, w, h)
    plane[rng.random((h, w)) < 0.15] = 100
    cells = np.argwhere((plane >= 0) & (plane <= 90))[::97, ::-1].astype(np.int32)
    nav = lom.NavField(RES, ORIGIN, w, h)
    nav.solve(plane, (50, 3, 400, 90, 1), cells)
    point_field = nav.potential()
    table = lom.navfieldCellCosts((50, 3, 400, 90, 1))
    goals = np.concatenate([cells, np.full((len(cells), 1), -1, np.int32)], axis=1)
    dev = lom.PoseField(RES, ORIGIN, w, h)
    for flags in (0, R.SPIN, BOTH):
        dev.solve(plane, ((50, 3, 400, 90, 1), 20, 1, 200, flags), S.POINT, goals)
        L = dev.layers()
        assert all(np.array_equal(L[hd], table[plane.view(np.uint8)]) for hd in range(8))
        floor = dev.floor()[0]
        # a pose route is a point route with turning costs on top: never cheaper, cell by cell
        assert (floor.astype(np.int64) >= point_field.astype(np.int64)).all()
        if flags & R.SPIN:
            assert np.array_equal(floor != R.UNREACHED, point_field != N.UNREACHED)
    assert (point_field != N.UNREACHED).sum() > 500


def test_layers_agree_with_the_rollouts_pose_test(lom):
    """L[h][cell] != 0 iff a rollout finds pose 0 free at (cell centre, 8192 h)"""
    w, h = 33, 31
    rng = np.random.default_rng(17)
    plane = S.with_unknown_and_invalid(rng, w, h)
    nav = N.params(50, 3, 400, 60)
    roll = lom.RolloutGrid(RES, ORIGIN, w, h)
    dev = lom.PoseField(RES, ORIGIN, w, h)
    rp = X.as_tuple(X.params(1, 1, lethal_min=nav["max_passable"] + 1, unknown_cost=-1))
    yy, xx = np.mgrid[0:h, 0:w]
    for fp_name in ("5x3", "L", "1024"):
        fp = FOOTPRINTS[fp_name]
        dev.solve(plane, R.as_tuple(R.params(nav, 0, 1, 0, 0)), fp, np.zeros((0, 3), np.int32))
        L = dev.layers()
        states = np.concatenate([np.stack([xx.ravel() * 32768 + 16384, yy.ravel() * 32768 + 16384, np.full(w * h, 8192 * hd)], axis=1)
                                 for hd in range(8)])
        free = []
        for first in range(0, len(states), 4096):                    # at most 4096 states a call
            roll.evaluate(plane, None, states[first:first + 4096], np.zeros((1, 1, 2), np.int16), fp, rp)
            free.append(roll.records()["free_poses"] >= 1)
        free = np.concatenate(free).reshape(8, h, w)
        assert np.array_equal(L != 0, free), fp_name
        assert 0 < free.sum() < free.size


def test_three_forms_the_chain_and_refused_producers(lom):
    import torch

    rng = np.random.default_rng(21)
    w, h = 90, 47
    occ = np.where(rng.random((h, w)) < 0.01, 100, 0).astype(np.int8)
    occ[rng.random((h, w)) < 0.02] = -1
    cp = K.params(1.0, 0.3, 1.5)
    clear = lom.ClearanceGrid(RES, ORIGIN, w, h)
    clear.update(occ, None, cp)
    cost = K.update(K.geometry(RES, ORIGIN[0], ORIGIN[1], w, h), occ, None, cp, table=lom.clearanceCostTable(cp, RES))["cost"]
    assert np.array_equal(clear.cost()[0], cost)
    p = R.params(NAV_UNKNOWN, 20, 2, 200, BOTH)
    fp = S.RECT_5x3
    goals = passable_goals(rng, layers_of(cost, p, fp), 3)
    ref = reference("chain", w, h, cost, p, fp, goals)
    assert 2 * ref["summary"]["states_reached"] >= ref["summary"]["states_reached"] + ref["summary"]["states_unreached"] > 1000
    a, b, c = (lom.PoseField(RES, ORIGIN, w, h) for _ in range(3))
    assert a.solve(cost, R.as_tuple(p), fp, goals) == ref["summary"]
    assert b.solveFromClearance(clear, R.as_tuple(p), fp, goals) == ref["summary"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        big = torch.ones(1 << 22, device="cuda:0")
        for _ in range(10):                                          # work in front of the plane
            big = big * 1.0001 + 1.0
        t_cost = torch.from_numpy(cost).to("cuda:0", non_blocking=True) + 0
        ev = torch.cuda.Event()
        ev.record(stream)
    assert c.solve(t_cost.data_ptr(), R.as_tuple(p), fp, goals, device=True, hip_event=C.c_void_p(ev.cuda_event)) == ref["summary"]
    for dev in (a, b, c):
        check_field(dev, ref, "forms")
    assert np.array_equal(clear.cost()[0], cost)                     # the producer goes on
    # the field keeps its own copy of the plane
    t_cost.fill_(100)
    torch.cuda.synchronize()
    check_paths_and_query(c, ref, p, rng, w, h, "device form")
    # the chain: ClearanceGrid -> PoseField -> RolloutGrid.evaluate_device with the floor as the potential
    table = lom.visibilityTable(X.TABLE)
    rfp = lom.rolloutFootprintRectangle(512, 512, 256, 128, False)
    free = np.argwhere(ref["floor"] != R.UNREACHED)
    pick = free[rng.choice(len(free), 6, replace=False)]
    states = np.stack([pick[:, 1] * 32768 + 16384, pick[:, 0] * 32768 + 16384, 8192 * ref["floor_heading"][tuple(pick.T)].astype(np.int64)], axis=1)
    cmd = np.stack([rng.integers(-6000, 12000, (150, 2)), rng.integers(-300, 300, (150, 2))], axis=2).astype(np.int16)
    xp = X.params(2, 30, 99, 30, min_steps=5, progress_weight=4, cost_weight=1, truncation_weight=100)
    want = X.evaluate_fast(cost, ref["floor"], states, cmd, rfp, table, xp)
    assert not want["error"] and want["summary"]["admissible"] > 50
    roll = lom.RolloutGrid(RES, ORIGIN, w, h)
    d_floor, d_heading = b.floorDevice()
    d_cost = C.c_void_p()
    assert lom.capi.lib().lom_clearance_cost_device(clear.handle, C.byref(d_cost)) == 0
    got = roll.evaluate(d_cost.value, d_floor, states, cmd, rfp, X.as_tuple(xp), device=True)
    assert got[1] == want["summary"] and got[0].tobytes() == want["picks"].tobytes() and roll.records().tobytes() == want["records"].tobytes()
    assert d_heading and b.potentialDevice()
    # a clearance grid of another geometry is refused, and nothing changes
    for other in (lom.ClearanceGrid(RES, ORIGIN, w + 1, h), lom.ClearanceGrid(RES, (ORIGIN[0] + 1e-6, ORIGIN[1]), w, h),
                  lom.ClearanceGrid(np.nextafter(np.float32(RES), np.float32(1)), ORIGIN, w, h)):
        with pytest.raises(lom.LomError) as e:
            b.solveFromClearance(other, R.as_tuple(p), fp, goals)
        assert e.value.code == lom.capi.ERR_ARG
    check_field(b, ref, "after refused producers")


# ---- 6: purity, refusals, shift ------------------------------------------------------------------------------------------------
def test_two_solves_agree_and_a_refused_call_changes_nothing(lom):
    rng = np.random.default_rng(30)
    w, h = 65, 33
    plane, nav = scenes_of(w, h)["sparse5"]
    fp, p = S.L_SHAPE, R.params(nav, 20, 2, 200, BOTH)
    goals = passable_goals(rng, layers_of(plane, p, fp), 5)
    dev = lom.PoseField(RES, ORIGIN, w, h)
    fl, fh = dev.floor()                                             # after create
    assert (dev.potential() == R.UNREACHED).all() and not dev.layers().any() and (fl == R.UNREACHED).all() and (fh == 8).all()
    assert dev.stats() == dict(launches=0, waits=0, tiles=0)
    ref = reference("purity", w, h, plane, p, fp, goals)
    first = dev.solve(plane, R.as_tuple(p), fp, goals)
    check_field(dev, ref, "first")
    dev.solve(S.serpentine(w, h), R.as_tuple(P_BOTH), S.POINT, np.array([(0, 0, -1)], np.int32))
    assert dev.potential().tobytes() != ref["P"].tobytes()
    assert dev.solve(plane, R.as_tuple(p), fp, goals) == first == ref["summary"]
    check_field(dev, ref, "again")
    starts = some_starts(rng, ref, w, h, 6)
    paths_before = dev.paths(starts, 20)
    L = lom.capi.lib()
    sm = lom.capi.PoseFieldSummary()
    g32, f32 = np.ascontiguousarray(goals, np.int32), np.ascontiguousarray(fp, np.int32)
    other = S.empty(w, h)
    good = lom.posefieldParams(R.as_tuple(p))
    nav_t = R.as_tuple(p)[0]
    bad_params = [(nav_t, R.MAX_COST + 1, 1, 0, 0), (nav_t, 0, R.MAX_COST + 1, 0, 0), (nav_t, 0, 1, R.MAX_COST + 1, 0), (nav_t, 0, 0, 0, R.SPIN),
                  (nav_t, 0, 1, 0, 4), ((0, 3, 400, 98, 0), 0, 1, 0, 0), ((50, 3, 400, 99, 0), 0, 1, 0, 0), ((50, 3, 0, 98, 1), 0, 1, 0, 0)]
    for bad in bad_params:
        sm.states_blocked = 9
        prm = lom.posefieldParams(bad)
        assert L.lom_posefield_solve(dev.handle, other.ctypes.data, C.byref(prm), f32.ctypes.data, len(f32), g32.ctypes.data, len(g32),
                                     C.byref(sm)) == lom.capi.ERR_ARG
        assert sm.asdict() == dict.fromkeys(R.SUMMARY_KEYS, 0) and L.lom_posefield_last_error(dev.handle)
    far = np.array([(16385, 0)], np.int32)
    for args in ((None, C.byref(good), f32.ctypes.data, len(f32), g32.ctypes.data, len(g32)),
                 (other.ctypes.data, None, f32.ctypes.data, len(f32), g32.ctypes.data, len(g32)),
                 (other.ctypes.data, C.byref(good), None, len(f32), g32.ctypes.data, len(g32)),
                 (other.ctypes.data, C.byref(good), f32.ctypes.data, 0, g32.ctypes.data, len(g32)),
                 (other.ctypes.data, C.byref(good), f32.ctypes.data, 1025, g32.ctypes.data, len(g32)),
                 (other.ctypes.data, C.byref(good), far.ctypes.data, 1, g32.ctypes.data, len(g32)),
                 (other.ctypes.data, C.byref(good), f32.ctypes.data, len(f32), None, 3),
                 (other.ctypes.data, C.byref(good), f32.ctypes.data, len(f32), g32.ctypes.data, (1 << 24) + 1)):
        sm.states_blocked = 9
        assert L.lom_posefield_solve(dev.handle, *args, C.byref(sm)) == lom.capi.ERR_ARG
        assert sm.asdict() == dict.fromkeys(R.SUMMARY_KEYS, 0)
    assert L.lom_posefield_solve_device(dev.handle, None, None, C.byref(good), f32.ctypes.data, len(f32), g32.ctypes.data, len(g32),
                                        C.byref(sm)) == lom.capi.ERR_ARG
    assert L.lom_posefield_solve_from_clearance(dev.handle, None, C.byref(good), f32.ctypes.data, len(f32), g32.ctypes.data, len(g32),
                                                C.byref(sm)) == lom.capi.ERR_ARG
    with pytest.raises(ValueError):
        dev.solve(plane[:-1], R.as_tuple(p), fp, goals)
    check_field(dev, ref, "after refused calls")                     # nothing changed
    after = dev.paths(starts, 20)
    assert after[0].tobytes() == paths_before[0].tobytes() and np.array_equal(after[1], paths_before[1])
    for option, bad in ((lom.capi.POSE_OPT_TEST_INNER_CAP, (1 << 20) + 1), (lom.capi.POSE_OPT_TEST_BATCH, 257),
                        (lom.capi.POSE_OPT_TEST_ALL_TILES, 2), (77, 0)):
        with pytest.raises(lom.LomError):
            dev.setOption(option, bad)
    # paths: a length above cap, cap 0, and the refusals
    far_start = starts[[int(np.argmax(paths_before[1]))]]
    states, lengths = dev.paths(far_start, 2)
    assert lengths[0] == paths_before[1].max() > 2 and states.tobytes() == R.paths(ref, p, far_start, 2)[0].tobytes()
    assert np.array_equal(dev.paths(starts, 0)[1], paths_before[1])
    assert L.lom_posefield_paths(dev.handle, None, 3, None, 0, None) == lom.capi.ERR_ARG
    assert L.lom_posefield_paths(dev.handle, starts.ctypes.data, len(starts), None, 4, None) == lom.capi.ERR_ARG
    assert L.lom_posefield_query(dev.handle, None, None, 3, None) == lom.capi.ERR_ARG
    few = np.full(50, 7, np.uint32)
    assert L.lom_posefield_potential(dev.handle, few.ctypes.data, 20) == 0
    assert np.array_equal(few[:20], ref["P"].ravel()[:20]) and (few[20:] == 7).all()
    assert dev.geometry() == dict(resolution=RES, origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=w, height=h)
    assert L.lom_posefield_device(dev.handle) == 0 and L.lom_posefield_stream(dev.handle)
    # shift: a fresh, cleared handle of the shifted geometry
    dev.shift(3, -2)
    want_geo = lom.grid_shift_geometry(geo_of(w, h), 3, -2)
    assert dev.geometry() == want_geo.asdict()
    fl, fh = dev.floor()
    assert (dev.potential() == R.UNREACHED).all() and not dev.layers().any() and (fl == R.UNREACHED).all() and (fh == 8).all()
    assert dev.paths(starts, 5)[1].sum() == 0
    assert (dev.query(np.array([[want_geo.origin_x + 1.0, want_geo.origin_y + 1.0]], np.float32), [-1]) == R.UNREACHED).all()
    fresh = lom.PoseField(RES, (want_geo.origin_x, want_geo.origin_y), w, h)
    assert dev.solve(plane, R.as_tuple(p), fp, goals) == fresh.solve(plane, R.as_tuple(p), fp, goals) == ref["summary"]
    check_field(dev, ref, "after the shift")
    dev.clear()
    assert (dev.potential() == R.UNREACHED).all() and not dev.layers().any()
    with pytest.raises(lom.LomError) as e:
        lom.PoseField(0.5, (0, 0), 10, 8193)
    assert e.value.code == lom.capi.ERR_ARG


# ---- mirrors -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::PoseField of the C++ mirror compiles with plain g++ and leaves the bytes the Python package leaves."""
    exe = cpp_program.build_with_library(tmp_path, "test_posefield_mirror.cpp")
    stdout = cpp_program.run(exe, "device", timeout=120)
    lines = stdout.strip().split("\n")
    got_summary = [int(v) for v in lines[-3].split()]
    got_field = np.array([int(v) for v in lines[-2].split()], np.uint64).astype(np.uint32)
    got_floor = np.array([int(v) for v in lines[-1].split()], np.uint64).astype(np.uint32)
    # the same grid, plane, footprint and goals here (tests/cpp/test_posefield_mirror.cpp)
    w, h = 45, 37
    i = np.arange(w * h)
    plane = np.where(i % 53 == 3, 100, np.where(i % 41 == 0, -1, (i % 11) * 7)).astype(np.int8).reshape(h, w)
    goals = np.array([(22, 18, -1), (5, 30, 2), (-1, 3, 0), (22, 18, 1)], np.int32)
    p = ((20, 2, 300, 80, 1), 15, 3, 100, 3)
    dev = lom.PoseField(RES, ORIGIN, w, h)
    summary = dev.solve(plane, p, S.RECT_5x3, goals)
    assert got_summary == [summary[k] for k in R.SUMMARY_KEYS]
    assert got_field.tobytes() == dev.potential().tobytes() and got_floor.tobytes() == dev.floor()[0].tobytes()
    assert summary["states_reached"] > 1000
