"""The trajectory rollouts without a GPU: the reference's two forms (tests/rollout_ref.py) against each other, the direction
table's symmetry, the motion's exactness along an axis and around a full circle, the library's host-only helpers against the
reference, a corridor scene whose outcome follows from its geometry, and the symbols of the ABI."""
import os
import re

import numpy as np
import pytest

from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import rollout_ref as R
from tests.rollout_scenes import commands_of
from tests.conftest import ROOT

CELL = 32768


@pytest.fixture(scope="module")
def table(lom):
    return lom.visibilityTable(R.TABLE)


# ---- the reference's two forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,segments,tn,f,unknown_cost,lethal_min,with_potential",
                         [(33, 31, 1, 20, 5, -1, 100, True), (20, 17, 3, 7, 1, 7, 50, False), (9, 40, 2, 33, 12, 7, 100, True),
                          (1, 1, 1, 1, 2, -1, 50, False)])
def test_the_two_forms_are_equal(table, w, h, segments, tn, f, unknown_cost, lethal_min, with_potential):
    rng = np.random.default_rng(w * 100 + h)
    plane = S.random_plane(rng, w, h, obstacles=0.05, unknown=0.1)
    potential = rng.integers(0, 5000, (h, w)).astype(np.uint32) if with_potential else None
    if with_potential:
        potential[rng.random((h, w)) < 0.1] = R.UNREACHED
    states = np.stack([rng.integers(-2 * CELL, (w + 2) * CELL, 6), rng.integers(-2 * CELL, (h + 2) * CELL, 6), rng.integers(0, 65536, 6)], axis=1)
    states[0] = (0, 0, 0)
    states[1] = (w * CELL - 1, h * CELL - 1, 65535)
    states[2] = (-1, 5, 100)                                                    # one unit outside: cell -1, invalid
    cmd = commands_of(rng, 9, segments)
    cmd[:, :, 0] //= 4                                                          # slow enough for some to stay inside
    fp = rng.integers(-400, 401, (f, 2))
    p = R.params(segments, tn, lethal_min, unknown_cost, min_steps=min(2, segments * tn), progress_weight=3, cost_weight=2, truncation_weight=5)
    slow, fast = R.evaluate(plane, potential, states, cmd, fp, table, p), R.evaluate_fast(plane, potential, states, cmd, fp, table, p)
    assert not slow["error"] and slow["summary"] == fast["summary"]
    assert slow["records"].tobytes() == fast["records"].tobytes() and slow["picks"].tobytes() == fast["picks"].tobytes()
    if w * h > 100:
        assert len(set(slow["records"]["reason"].tolist())) >= 3 and slow["summary"]["valid_states"] < 6


def test_a_refused_reference_call_is_empty(table):
    plane = S.empty(4, 4)
    for p, states in ((R.params(9, 1), [(0, 0, 0)]), (R.params(8, 128, min_steps=1025), [(0, 0, 0)]), (R.params(1, 1), [(1 << 29, 0, 0)]),
                      (R.params(1, 1), [(0, 0, 65536)])):
        got = R.evaluate_fast(plane, None, states, np.zeros((1, p["segments"], 2), np.int16), [(0, 0)], table, p)
        assert got["error"] and got["summary"] == dict.fromkeys(R.SUMMARY_KEYS, 0) and not got["picks"]["k"].any()


# ---- the table and the motion ------------------------------------------------------------------------------------------------
def test_the_table_is_antisymmetric_and_near_numpys(table):
    assert table.shape == (R.TABLE, 2) and table.dtype == np.int32
    assert np.array_equal(table[: R.TABLE // 2], -table[R.TABLE // 2:])
    assert np.abs(table.astype(np.int64) - R.numpy_table()).max() <= 1
    assert table[0].tolist() == [32768, 0] and table[R.TABLE // 4].tolist() == [0, 32768]


def test_a_straight_run_along_x_is_exact(lom, table):
    p = R.params(2, 50)
    got = lom.rolloutPoses(R.as_tuple(p), (123, -456, 0), [(32767, 0), (32767, 0)])
    assert np.array_equal(got[:, 0], 123 + 32767 * np.arange(101)) and (got[:, 1] == -456).all() and (got[:, 2] == 0).all()
    assert got.tolist() == [list(q) for q in R.poses(p, (123, -456, 0), [(32767, 0), (32767, 0)], table)]


@pytest.mark.parametrize("v,w", [(32767, 64), (20000, 256), (-32767, -128)])
def test_a_full_circle_returns(lom, table, v, w):
    """|w| is a multiple of 16 that divides 65536, so the N = 65536 / |w| steps read N equally spaced entries of the table,
    which sum to zero by its antisymmetry; each increment rounds by at most half a unit: within N / 2 units per axis."""
    n = 65536 // abs(w)
    assert abs(w) % 16 == 0 and n * abs(w) == 65536 and n <= 1024
    tn = 128 if n % 128 == 0 else n
    p, cmd = R.params(n // tn, tn), [(v, w)] * (n // tn)                        # one command, repeated over the segments
    start = (5 * CELL + 17, -3 * CELL + 5, 4096)
    got = lom.rolloutPoses(R.as_tuple(p), start, cmd)
    assert got.tolist() == [list(q) for q in R.poses(p, start, cmd, table)]
    assert got[-1, 2] == start[2] and abs(got[-1, 0] - start[0]) <= n // 2 and abs(got[-1, 1] - start[1]) <= n // 2
    assert np.abs(got[n // 2, :2] - got[0, :2]).max() > abs(v) * n // 8         # it did go round


def test_poses_refuses_bad_arguments(lom):
    for p, state in ((R.params(0, 1), (0, 0, 0)), (R.params(8, 129), (0, 0, 0)), (R.params(1, 1), (-(1 << 29) - 1, 0, 0)),
                     (R.params(1, 1), (0, 0, 65536))):
        with pytest.raises(lom.LomError):
            lom.rolloutPoses(R.as_tuple(p), state, np.zeros((max(p["segments"], 1), 2), np.int16))


# ---- the helpers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front,back,half,spacing", [(1280, 1280, 768, 256), (1000, 300, 500, 300), (0, 0, 0, 1), (16384, 16384, 16384, 2048),
                                                     (5, 0, 3, 7), (700, 700, 10, 64)])
def test_footprint_rectangle(lom, front, back, half, spacing):
    filled, border = lom.rolloutFootprintRectangle(front, back, half, spacing), lom.rolloutFootprintRectangle(front, back, half, spacing, True)
    assert filled.dtype == np.int32 and np.array_equal(filled, R.footprint_rectangle(front, back, half, spacing))
    assert np.array_equal(border, R.footprint_rectangle(front, back, half, spacing, True))
    nx, ny = -(-(front + back) // spacing) + 1, -(-2 * half // spacing) + 1
    assert len(filled) == nx * ny and len(border) == (nx * ny if min(nx, ny) <= 2 else 2 * nx + 2 * ny - 4)
    points = set(map(tuple, filled.tolist()))
    assert len(points) == len(filled) and set(map(tuple, border.tolist())) <= points
    if 2 * half % spacing == 0 or 2 * half <= spacing:                          # the lattice ends on the far side by itself:
        assert {(x, -y) for x, y in points} == points                           # symmetric about the robot's axis
    assert {y for _, y in points} >= {-half, half} and {(x, y) for x, y in points if abs(y) == half} == {(x, -y) for x, y in points if abs(y) == half}
    assert filled[:, 0].min() == -back and filled[:, 0].max() == front and filled[:, 1].min() == -half and filled[:, 1].max() == half
    for x, y in border.tolist():
        assert x in (-back, front) or y in (-half, half)


def test_footprint_rectangle_refusals(lom):
    for args in ((-1, 0, 0, 1), (0, 16385, 0, 1), (0, 0, 16385, 1), (10, 10, 10, 0), (4096, 4096, 4096, 128)):
        with pytest.raises(lom.LomError):
            lom.rolloutFootprintRectangle(*args)
    assert len(lom.rolloutFootprintRectangle(4096, 4096, 4096, 128, True)) == 2 * 65 + 2 * 65 - 4


def test_state_from_pose_against_numpy(lom):
    rng = np.random.default_rng(5)
    geo = N.geometry(0.1, -5.0, 3.25, 100, 80)
    tup = (geo["resolution"], geo["origin_x"], geo["origin_y"], geo["width"], geo["height"])
    cases = [(0.0, 0.0, 0.0), (-5.0, 3.25, np.pi), (-5.05, 3.2, -np.pi), (4.99, 11.2, 2 * np.pi), (1.0, 2.0, -1e-6), (1.0, 2.0, 100.0)]
    cases += [tuple(v) for v in np.concatenate([rng.uniform(-20, 20, (50, 2)), rng.uniform(-10, 10, (50, 1))], axis=1)]
    for x, y, yaw in cases:
        assert lom.rolloutStateFromPose(tup, x, y, yaw) == R.state_from_pose(geo, x, y, yaw), (x, y, yaw)
    assert lom.rolloutStateFromPose(tup, -5.05, 3.25, 0.0)[0] < 0               # the floor rule
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, np.nan), (1e6, 0, 0), (0, -1e6, 0)):
        assert R.state_from_pose(geo, *bad) is None
        with pytest.raises(lom.LomError):
            lom.rolloutStateFromPose(tup, *bad)


# ---- a corridor with a wall ahead and a way out to the left ---------------------------------------------------------------------
def corridor():
    """60 x 41: a corridor along x over rows 7 .. 13, closed by a wall at column 40, with a side corridor up columns 27 .. 39"""
    plane = np.full((41, 60), 100, np.int8)
    plane[7:14, :40] = 0
    plane[14:, 27:40] = 0
    return plane


def test_corridor_with_a_wall_ahead(table):
    plane = corridor()
    geo = N.geometry(0.1, 0.0, 0.0, 60, 41)
    potential = N.solve(geo, plane, N.params(50, 0, 1, 98), np.array([[33, 38]], np.int32))["P"]
    fp = R.footprint_rectangle(512, 256, 256, 256)                              # 2 cells ahead, 1 behind, 1 to each side
    state = (10 * CELL + CELL // 2, 10 * CELL + CELL // 2, 0)
    cmd = np.array([[(16384, 0), (16384, 0)], [(32767, 0), (32767, 0)], [(16384, 0), (16384, 512)], [(0, 0), (0, 0)],
                    [(16384, 0), (16384, -512)]], np.int16)
    p = R.params(2, 32, min_steps=0, progress_weight=1, cost_weight=1, truncation_weight=100)
    got = R.evaluate(plane, potential, [state], cmd, fp, table, p)
    assert got == _same_as(R.evaluate_fast(plane, potential, [state], cmd, fp, table, p), got)
    rec = got["records"]
    # heading 0 reads (32768, 0): a step adds (v * 32768 + 16384) >> 15 = v units, the front samples lie 2 cells ahead, and
    # the wall's first cell is 40: the first blocked pose is the least t with x0 + v t + 2 cells >= 40 cells
    for k, v in ((0, 16384), (1, 32767)):
        want = -(-(40 * CELL - 2 * CELL - state[0]) // v)
        assert rec["free_poses"][k] == want and rec["reason"][k] == R.COLLISION, (k, want, rec[k])
        assert rec["end_x"][k] == state[0] + v * (want - 1) and rec["end_y"][k] == state[1] and rec["end_angle"][k] == 0
    assert rec["free_poses"][3] == 65 and rec["end_potential"][3] == potential[10, 10]          # standing still
    assert rec["free_poses"][4] < 65 and rec["reason"][4] == R.COLLISION                        # right, into the wall
    assert rec["free_poses"][2] == 65 and rec["end_angle"][2] == 16384                          # left, a quarter turn
    pick = got["picks"][0]
    assert pick["k"] == 2 and pick["admissible"] == 5 and rec["end_potential"][2] < potential[10, 10]
    assert pick["score"] == int(potential[10, 10]) - int(rec["end_potential"][2]) - int(rec["cost_sum"][2])
    # without a potential nothing rewards motion: the two that lose no pose gather no cost and tie at 0; ties go to the least k
    alone = R.evaluate(plane, None, [state], cmd, fp, table, p)
    assert alone["picks"]["k"][0] == 2 and alone["picks"]["score"][0] == 0 and (alone["records"]["end_potential"] == R.UNREACHED).all()
    # min_steps = S: only the candidates that lose no pose remain
    strict = R.evaluate(plane, potential, [state], cmd, fp, table, dict(p, min_steps=64))
    assert strict["picks"]["admissible"][0] == 2 and strict["picks"]["k"][0] == 2


def _same_as(a, b):
    assert a["records"].tobytes() == b["records"].tobytes() and a["picks"].tobytes() == b["picks"].tobytes() and a["summary"] == b["summary"]
    return b


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_every_declared_symbol_is_exported_and_bound(lom):
    header = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    declared = set(re.findall(r"\b(lom_rollout_[a-z_]+)\s*\(", header))
    assert len(declared) == 17 and declared <= set(lom.capi.EXPORTED)
    L = lom.capi.lib()
    assert all(hasattr(L, s) for s in declared)
    assert re.search(r"#define LOM_ROLLOUT_TABLE 4096\b", header) and lom.capi.ROLLOUT_TABLE == R.TABLE == 4096
