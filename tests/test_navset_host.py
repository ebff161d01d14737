"""tests/navset_ref.py on its own, no GPU: the potential of nearest() equals the single solve from the union of the goals,
gather() equals indexing, the owner is the least index among equals, and the travel-cost matrix is not symmetric where two
end cells cost differently (a step pays for the cell it leaves)."""
import numpy as np
import pytest

from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import navset_ref as NS

P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)
W, H = 33, 31


def geo_of(w, h):
    return N.geometry(0.25, -3.0, 2.0, w, h)


def scenes():
    rng = np.random.default_rng(5)
    rnd = S.random_plane(rng, W, H)
    return {"empty": (S.empty(W, H), P0), "random": (rnd, P0), "random_unknown_passable": (rnd, P1), "serpentine": (S.serpentine(W, H), P0),
            "spiral": (S.spiral(W, H), P0), "diagonal_gaps": (S.diagonal_gaps(W, H), P0), "pocket": (S.pocket(W, H), P0),
            "two_rooms": (S.two_rooms(W, H, 7), P0), "all_blocked": (np.full((H, W), 100, np.int8), P0)}


def goal_sets(rng, plane):
    """five fields: three random goals each, one with none, one that shares a goal with the first"""
    free = np.argwhere((plane >= 0) & (plane <= 90))[:, ::-1]
    pick = lambda n: free[rng.integers(0, len(free), n)] if len(free) else np.array([(0, 0)] * n)
    a = pick(3)
    return [a, pick(3), np.zeros((0, 2), np.int64), np.concatenate([a[:1], pick(2)]), np.array([(W - 1, H - 1), (-1, 0)])]


@pytest.mark.parametrize("name", list(scenes()))
def test_nearest_is_the_solve_from_the_union_and_gather_is_indexing(name):
    plane, p = scenes()[name]
    rng = np.random.default_rng(len(name))
    geo = geo_of(W, H)
    goals = goal_sets(rng, plane)
    fields = NS.solve_set(geo, plane, p, goals)
    owner, potential, owned = NS.nearest(geo, fields)
    union = N.solve(geo, plane, p, np.concatenate(goals))
    assert potential.tobytes() == union["P"].tobytes()
    assert ((owner == NS.NO_OWNER) == (union["P"] == N.UNREACHED)).all()
    assert int(owned.sum()) == union["summary"]["cells_reached"] and owned[2] == 0
    # the owner attains the least value, and no field of a lower index does
    for i, f in enumerate(fields):
        mine = owner == i
        assert (f["P"][mine] == potential[mine]).all()
        assert not ((f["P"] == potential) & (owner > i) & (owner != NS.NO_OWNER)).any()
    # gather: indexing, unreached outside the grid
    pts = np.concatenate([rng.integers(0, [W, H], (20, 2)), [(-1, 3), (W, 0), (0, H), (5, -2)]])
    got = NS.gather(geo, fields, pts)
    assert got.shape == (5, 24) and (got[:, 20:] == N.UNREACHED).all()
    for i, f in enumerate(fields):
        assert (got[i, :20] == f["P"][pts[:20, 1], pts[:20, 0]]).all()
    assert NS.gather(geo, fields, np.zeros((0, 2), np.int32)).shape == (5, 0)
    assert NS.gather(geo, [], pts).shape == (0, 24)


def test_gather_in_metres_uses_the_floor_rule():
    geo = geo_of(W, H)
    fields = NS.solve_set(geo, S.empty(W, H), P0, [np.array([(0, 0)]), np.array([(W - 1, H - 1)])])
    xy = np.array([[-3.0, 2.0], [-2.75, 2.25], [-3.0000002, 2.0], [np.nan, 2.0], [5.2, 9.7]], np.float32)
    got = NS.gather(geo, fields, xy, metres=True)
    assert got[0, 0] == 0 and got[0, 1] == 7 * 50 and (got[:, 2:4] == N.UNREACHED).all()
    assert got[1, 4] == fields[1]["P"][30, 32] == 0


def test_the_travel_cost_matrix_is_not_symmetric_over_a_costly_cell():
    """Two goals on a corridor; the cell of goal B costs more than A's.  A step pays for the cell it leaves: the way from B
    to A leaves B and pays for it, the way from A to B never does."""
    plane = np.zeros((1, 6), np.int8)
    plane[0, 4] = 60                                        # goal B's cell: 50 + 3 * 60 = 230 per unit, against 50
    geo = geo_of(6, 1)
    a, b = (1, 0), (4, 0)
    fields = NS.solve_set(geo, plane, P0, [np.array([a]), np.array([b])])
    m = NS.gather(geo, fields, np.array([a, b]))            # m[i, j]: from goal j to goal i
    assert m[0, 0] == 0 and m[1, 1] == 0
    assert m[0, 1] == 5 * 230 + 2 * 5 * 50                  # from B to A: leaves B, then two free cells
    assert m[1, 0] == 3 * 5 * 50                            # from A to B: leaves three free cells, never B
    assert m[0, 1] != m[1, 0]


def test_offsets_rule():
    ok = NS.offsets_ok
    assert ok(None, 0, 4) and ok([0, 0], 1, 1) and ok([0, 2, 2, 5], 3, 3) and ok([0, 1 << 24], 1, 1)
    assert not ok([0, 1, 2], 2, 1)                                  # more fields than the set holds
    assert not ok(None, 1, 4) and not ok([1, 2], 1, 4)              # no offsets; a start that is not 0
    assert not ok([0, 3, 2], 2, 4)                                  # falls
    assert not ok([0, (1 << 24) + 1], 1, 4)                         # too many goals
    assert not ok([0, 1], 1, 4, have_goals=False) and ok([0, 0], 1, 4, have_goals=False)
    goals, offsets = NS.offsets_of([np.array([(1, 2), (3, 4)]), np.zeros((0, 2), np.int32), np.array([(5, 6)])])
    assert offsets.tolist() == [0, 2, 2, 3] and goals.tolist() == [[1, 2], [3, 4], [5, 6]]
