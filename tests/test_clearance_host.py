"""Clearance grid, the parts that need no GPU: the reference (tests/clearance_ref.py) against a brute-force distance and
against scipy, the merge truth table, the cost table against the library's, the corridor scene on the reference alone, the
declarations and the refusals that touch no device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import occupancy_scene as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_clearance_create", "lom_clearance_destroy", "lom_clearance_last_error", "lom_clearance_clear",
               "lom_clearance_get_geometry", "lom_clearance_stream", "lom_clearance_device", "lom_clearance_wait_event",
               "lom_clearance_set_option", "lom_clearance_update", "lom_clearance_update_device",
               "lom_clearance_update_from_grids", "lom_clearance_cost", "lom_clearance_cost_device", "lom_clearance_distance_sq",
               "lom_clearance_distance", "lom_clearance_cost_table", "lom_clearance_query"]


# ---- the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_separable_distance_equals_all_pairs(seed):
    rng = np.random.default_rng(seed)
    h, w = rng.integers(1, 25, 2)
    ob = rng.random((h, w)) < (0.0, 0.02, 0.05, 0.2, 0.5, 1.0)[seed]
    if seed == 1:
        ob[rng.integers(h), rng.integers(w)] = True
    for R in (0, 1, 2, 5, 7, 40):
        got, want = K.distance_sq(ob, R), K.brute_distance_sq(ob, R)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (R, np.argwhere(got != want)[:5])
        assert ((got == 0) == ob).all() and ((got <= R * R) | (got == K.FAR)).all()


def test_distance_equals_scipy_where_the_radius_covers_the_grid():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    ob = rng.random((67, 130)) < 0.004
    assert ob.sum() >= 3
    edt = np.rint(ndimage.distance_transform_edt(~ob) ** 2).astype(np.int64)
    for R in (150, 40, 7):                                       # 150 covers the grid's diagonal: nothing is far
        got = K.distance_sq(ob, R)
        assert np.array_equal(got, np.where(edt <= R * R, edt, K.FAR).astype(np.uint16))
        assert R == 40 or (got == K.FAR).any() == (R == 7)


def test_merge_truth_table():
    o_vals, e_vals = [-1, 0, 100, 1, 50, -2, 127, -128], [-1, 0, 1, 57, 99, 100, 101, 127, -2, -128]
    occ, elev = (a.astype(np.int8) for a in np.meshgrid(o_vals, e_vals, indexing="ij"))
    for flags in range(4):
        base, ob, invalid, cleared = K.merge(occ, elev, flags)
        for i, o in enumerate(o_vals):
            for j, e in enumerate(e_vals):
                bad = o not in (-1, 0, 100) or not -1 <= e <= 100
                oo, ee = (o if o in (-1, 0, 100) else -1), (e if -1 <= e <= 100 else -1)
                clr = ee == 100 and bool(flags & 1) and oo == 0
                lethal_e = ee == 100 and not clr
                want = 100 if (oo == 100 or lethal_e) else ((0 if clr else ee) if (0 <= ee <= 99 or clr) else (0 if oo == 0 else -1))
                assert (base[i, j], invalid[i, j], cleared[i, j]) == (want, bad, clr), (flags, o, e)
                assert ob[i, j] == (want == 100 or (want == -1 and bool(flags & 2)))
    # a plane left out reads as all -1
    b0, ob0, _, _ = K.merge(None, elev, 0)
    b1, ob1, _, _ = K.merge(np.full_like(occ, -1), elev, 0)
    assert np.array_equal(b0, b1) and np.array_equal(ob0, ob1)
    assert (K.merge(occ, None, 3)[0] == np.where(np.isin(occ, (0, 100)), occ, -1)).all()


def test_cost_and_summary_by_hand():
    geo = K.geometry(0.5, 0.0, 0.0, 9, 1)
    p = K.params(1.6, 0.5, 1.0)                                   # R = 3; table: 100, 99 (0.5 m), then the decay at 1.0, 1.5 m
    t = K.cost_table(p, 0.5)
    assert K.radius_cells(p, 0.5) == 3 and len(t) == 10 and t[0] == 100 and t[1] == 99
    assert t[4] == int(np.floor(98 * np.exp(-0.5))) and t[9] == int(np.floor(98 * np.exp(-1.0))) and (np.diff(t.astype(int)) <= 0).all()
    occ = np.array([[100, 0, 0, 0, 0, -1, -1, -1, -1]], np.int8)
    elev = np.array([[-1, -1, 70, -1, -1, -1, -1, -1, 30]], np.int8)
    r = K.update(geo, occ, elev, p)
    assert r["d2"].tolist() == [[0, 1, 4, 9, K.FAR, K.FAR, K.FAR, K.FAR, K.FAR]]
    assert r["cost"].tolist() == [[100, 99, 70, t[9], 0, -1, -1, -1, 30]]             # max(base, c); unknown stays unknown when far
    assert r["summary"] == dict(cells_lethal=1, cells_inscribed=1, cells_costed=4, cells_unknown=3, cells_invalid=0, cells_cleared=0)
    r = K.update(geo, occ, elev, K.params(1.6, 0.5, 1.0, K.UNKNOWN_IS_OBSTACLE))
    assert r["cost"].tolist() == [[100, 99, 70, t[4], 99, 100, 100, 100, 99]]         # unknown cells are obstacles now
    assert K.metres(r["d2"], 0.5).tolist() == [[0.0, 0.5, 1.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0.5]]
    near = K.update(geo, np.array([[100, -1, -1, -1, -1, -1, -1, -1, -1]], np.int8), None, p)
    assert near["cost"].tolist() == [[100, 99, t[4], t[9], -1, -1, -1, -1, -1]]       # an unknown cell near an obstacle takes c
    # a window rewrites its cells only, and sees the obstacle outside it
    w = K.update(geo, occ, elev, p, window=(1, -3, 2, 9))
    assert w["d2"].tolist() == [[K.FAR, 1, 4] + [K.FAR] * 6] and w["cost"].tolist() == [[-1, 99, 70] + [-1] * 6]
    assert w["summary"]["cells_inscribed"] == 1 and sum(w["summary"].values()) == 2
    assert K.update(geo, occ, elev, p, window=(9, 0, 3, 3))["summary"] == dict.fromkeys(K.SUMMARY_KEYS, 0)
    assert K.update(geo, None, None, p)["error"] and K.update(geo, occ, None, K.params(1.0, 2.0, 1.0))["error"]
    d, c = K.query(geo, r["d2"], r["cost"], [[0.49, 0.2], [0.5, 0.0], [-0.01, 0.2], [4.4, 0.5], [np.nan, 0.1], [1.2, -1e-6]])
    assert c.tolist() == [100, 99, -1, -1, -1, -1] and d[:2].tolist() == [0.0, 0.5] and np.isnan(d[2:]).all()


# ---- the scene -----------------------------------------------------------------------------------------------------------------
SCENE_PARAMS = K.params(inflation_radius=15.0, inscribed_radius=0.75, decay=0.5)


def scene_measures():
    occ = OS.reference(True)["cls"]
    r = K.update(OS.GEO, occ, None, SCENE_PARAMS)
    m = K.metres(r["d2"], OS.RES)
    X, Y = OS.centres()
    row = int(np.argmin(np.abs(Y[:, 0] - OS.RES / 2)))           # the row just above y = 0: the corridor's centre line
    cols = (X[0] > OS.X_LO) & (X[0] < OS.X_HI)
    line = m[row, cols]
    co = OS.corridor_mask()
    inscribed = float(np.float32(SCENE_PARAMS["inscribed_radius"]))
    return dict(centre_cells=int(cols.sum()), centre_clearance_median=float(np.median(line)), centre_clearance_min=float(line.min()),
                centre_far=float(np.isinf(line).mean()), corridor_cells=int(co.sum()),
                corridor_below_inscribed=float((m[co] <= inscribed).mean()), corridor_lethal=float((r["cost"][co] == 100).mean()),
                summary=r["summary"])


def test_corridor_scene_on_the_reference_alone():
    """The corridor of tests/vote_scene.py, classified by tests/occupancy_ref.py (with the mover), through
    tests/clearance_ref.py at 15 m inflation and 0.75 m inscribed radius.  Figures of this reference
    (profiles/clearance_scene.json, written here): along the centre line (180 cells) the clearance has the median
    11.75 m -- the walls stand at +-12 m -- and the minimum 6.5 m, beside a box; no cell of it is far; 4.95 % of the 16,560
    corridor cells lie within the inscribed radius of an obstacle and 0.085 % are lethal (the occupied share of 7j)."""
    m = scene_measures()
    out = os.path.join(ROOT, "profiles", "clearance_scene.json")
    try:
        with open(out, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass  # (a read-only tree: the figures are printed all the same)
    print("clearance scene:", m)
    assert m["centre_cells"] == 180 and m["corridor_cells"] == 16560
    # the loose bounds, chosen from the figures above
    assert 11.0 <= m["centre_clearance_median"] <= 12.0 and 5.0 <= m["centre_clearance_min"] <= 8.0 and m["centre_far"] == 0.0
    assert 0.02 <= m["corridor_below_inscribed"] <= 0.10 and m["corridor_lethal"] <= 0.005
    # the recorded figures
    assert m["centre_clearance_median"] == 11.75 and m["centre_clearance_min"] == 6.5
    assert round(m["corridor_below_inscribed"], 4) == 0.0495 and round(m["corridor_lethal"], 5) == 0.00085
    assert m["summary"] == dict(cells_lethal=1020, cells_inscribed=5895, cells_costed=54823, cells_unknown=8342, cells_invalid=0,
                                cells_cleared=0)
    assert sum(m["summary"].values()) == OS.GEO["width"] * OS.GEO["height"]


# ---- declarations and refusals -----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"clearance grid", text) and re.search(r"#define LOM_CLEAR_FAR 65535", text)
    assert re.search(r"LOM_CLEAR_OPT_TEST_TILE_ROWS\s*=\s*1", text) and re.search(r"LOM_CLEAR_OPT_TEST_NO_PRUNE\s*=\s*2", text)
    assert re.search(r"LOM_CLEAR_FREE_CLEARS_ELEVATION\s*=\s*1", text) and re.search(r"LOM_CLEAR_UNKNOWN_IS_OBSTACLE\s*=\s*2", text)
    assert lom.capi.lib().lom_abi_version() == 2
    assert (lom.capi.CLEAR_FAR, lom.capi.CLEAR_FREE_CLEARS_ELEVATION, lom.capi.CLEAR_UNKNOWN_IS_OBSTACLE) == \
        (K.FAR, K.FREE_CLEARS_ELEVATION, K.UNKNOWN_IS_OBSTACLE)
    for name, size in dict(ClearanceParams=16, ClearanceWindow=16, ClearanceSummary=48).items():
        assert C.sizeof(getattr(lom.capi, name)) == size, name
    assert [k for k, _ in lom.capi.ClearanceSummary._fields_] == list(K.SUMMARY_KEYS)
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    names = ("update", "updateFromGrids", "cost", "distance", "distanceSq", "query", "clear", "setOption")
    assert re.search(r"class ClearanceGrid", mirror) and re.search(r"\bclearanceParams\s*\(", mirror)
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert hasattr(lom.ClearanceGrid, name), name
    assert lom.clearanceParams((2.0, 0.5, 1.0, 3)).flags == 3


@pytest.mark.parametrize("p,res", [((2.0, 0.5, 1.5, 0), 0.25), ((5.0, 0.0, 0.0, 0), 0.25), ((1.0, 1.0, 3.0, 0), 0.1), ((0.1, 0.05, 1.0, 0), 0.25),
                                   ((25.4, 3.0, 0.2, 0), 0.1), ((3.3, 0.7, 7.5, 2), 0.05)])
def test_cost_table_of_the_library(lom, p, res):
    got = lom.clearanceCostTable(p, res)
    kp = K.params(*p)
    R = K.radius_cells(kp, res)
    assert len(got) == R * R + 1
    K.compare_table(got, kp, res)
    # the cap, and no output at all
    L = lom.capi.lib()
    cp, geo = lom.clearanceParams(p), lom.capi.OccupancyGeometry(res, 0.0, 0.0, 3, 3)
    few = np.full(8, 7, np.uint8)
    assert L.lom_clearance_cost_table(C.byref(cp), C.byref(geo), few.ctypes.data, min(4, len(got))) == len(got)
    assert np.array_equal(few[:min(4, len(got))], got[:4]) and (few[4:] == 7).all()


def test_bad_arguments_are_refused_without_a_device(lom):
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    h = C.c_void_p()
    good = dict(resolution=0.25, origin_x=0.0, origin_y=0.0, width=10, height=10)
    for change in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=np.nan), dict(resolution=np.inf),
                   dict(origin_x=np.nan), dict(origin_y=np.inf), dict(width=0), dict(height=0), dict(width=8193), dict(height=8193)):
        geo = lom.capi.OccupancyGeometry(**dict(good, **change))
        assert L.lom_clearance_create(C.byref(geo), 0, C.byref(h)) == ERR_ARG, change
        assert b"geometry" in L.lom_clearance_last_error(None)
        assert L.lom_clearance_cost_table(C.byref(lom.clearanceParams((1.0, 0.5, 1.0, 0))), C.byref(geo), None, 0) == ERR_ARG
    assert L.lom_clearance_create(None, 0, C.byref(h)) == ERR_ARG
    geo = lom.capi.OccupancyGeometry(**good)
    assert L.lom_clearance_create(C.byref(geo), 0, None) == ERR_ARG
    # parameters, through the one entry that needs no handle: R > 254, inscribed > inflation, negative, not finite, flags
    for bad in ((63.75, 0.5, 1.0, 0), (1.0, 1.5, 1.0, 0), (-1.0, -2.0, 1.0, 0), (1.0, -0.5, 1.0, 0), (1.0, 0.5, -1.0, 0),
                (np.nan, 0.5, 1.0, 0), (1.0, np.nan, 1.0, 0), (1.0, 0.5, np.nan, 0), (np.inf, 0.5, 1.0, 0), (1.0, 0.5, np.inf, 0),
                (1.0, 0.5, 1.0, 4)):
        assert L.lom_clearance_cost_table(C.byref(lom.clearanceParams(bad)), C.byref(geo), None, 0) == ERR_ARG, bad
        assert not K.params_ok(K.params(*bad), 0.25), bad
        with pytest.raises(lom.LomError):
            lom.clearanceCostTable(bad, 0.25)
    assert L.lom_clearance_cost_table(C.byref(lom.clearanceParams((63.5, 0.5, 1.0, 0))), C.byref(geo), None, 0) == 254 * 254 + 1
    assert L.lom_clearance_cost_table(None, C.byref(geo), None, 0) == ERR_ARG
    assert L.lom_clearance_cost_table(C.byref(lom.clearanceParams((1.0, 0.5, 1.0, 0))), C.byref(geo), None, 5) == ERR_ARG
    # NULL handles; the summary is zeroed
    prm, plane = lom.clearanceParams((1.0, 0.5, 1.0, 0)), np.zeros(100, np.int8)
    sm = lom.capi.ClearanceSummary()

    def zeroed(rc):
        ok = rc == ERR_ARG and sm.asdict() == dict.fromkeys(K.SUMMARY_KEYS, 0)
        sm.cells_lethal = sm.cells_cleared = 5
        return ok

    sm.cells_lethal = sm.cells_cleared = 5
    assert zeroed(L.lom_clearance_update(None, plane.ctypes.data, plane.ctypes.data, C.byref(prm), None, C.byref(sm)))
    assert zeroed(L.lom_clearance_update(None, None, None, C.byref(prm), None, C.byref(sm)))
    assert zeroed(L.lom_clearance_update_device(None, None, None, None, C.byref(prm), None, C.byref(sm)))
    assert zeroed(L.lom_clearance_update_from_grids(None, None, None, None, None, None, C.byref(prm), None, C.byref(sm)))
    assert zeroed(L.lom_clearance_cost(None, None, 0, C.byref(sm)))
    assert L.lom_clearance_cost_device(None, C.byref(h)) == ERR_ARG
    assert L.lom_clearance_distance_sq(None, None, 0) == ERR_ARG and L.lom_clearance_distance(None, None, 0) == ERR_ARG
    assert L.lom_clearance_query(None, None, 0, None, None) == ERR_ARG
    assert L.lom_clearance_clear(None) == ERR_ARG and L.lom_clearance_device(None) == ERR_ARG
    assert L.lom_clearance_get_geometry(None, None) == ERR_ARG and L.lom_clearance_wait_event(None, None) == ERR_ARG
    assert L.lom_clearance_set_option(None, 1, 1) == ERR_ARG and L.lom_clearance_stream(None) is None
    L.lom_clearance_destroy(None)
    with pytest.raises(TypeError):
        lom.clearanceParams(dict(inflation_radius=1.0))  # no defaults: all four fields or none
