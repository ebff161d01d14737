"""Elevation grid, the parts that need no GPU: the reference (tests/elevation_ref.py) by hand -- quantisation, the height
limit, the accumulators, the exact plane fit, the cost's branches -- the ramp / kerb / wall / beam scene on the reference
alone, the declarations and the refusals that touch no device."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

from tests import elevation_ref as E
from tests import elevation_scene as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_elevation_create", "lom_elevation_destroy", "lom_elevation_last_error", "lom_elevation_clear",
               "lom_elevation_get_geometry", "lom_elevation_stream", "lom_elevation_device", "lom_elevation_wait_event",
               "lom_elevation_set_option", "lom_elevation_integrate", "lom_elevation_integrate_cloud",
               "lom_elevation_integrate_cloud_device", "lom_elevation_cells", "lom_elevation_layers", "lom_elevation_cost",
               "lom_elevation_cost_device", "lom_odometry_elevation_scan"]
IDENT = [0, 0, 0, 1, 0, 0, 0]


# ---- the reference by hand ---------------------------------------------------------------------------------------------------
def test_quantisation_height_limit_and_accumulators():
    geo = E.geometry(0.5, 0.0, 0.0, 8, 4, 0.5)
    p = E.point_params(-4000.0, 4000.0, 0.5, 4000.0)
    Q = E.Q
    z = [0.5, 0.5 + 0.5 * Q, 0.5 + 1.5 * Q, 0.5 + 2.5 * Q, 0.5 - 0.5 * Q, 0.5 - 1.5 * Q,   # ties: to even
         2048.5, -2047.5, 2048.5 - 2.0 ** -12, -2047.5 + 2.0 ** -12,                       # |h| = 2048 is out, just inside is in
         1.0, 1.0, -3.0]
    pts = np.array([[1.25, 0.75, v] for v in z], np.float32)
    assert [float(v) for v in pts[:, 2]] == z                                               # every height is an f32
    pose = [0.1, 0.1, 0.0, 1, 0, 0, 0]
    c, zq, n_out = E.scan_points(geo, pose, pts - np.float32([0.1, 0.1, 0.0]), p)
    assert zq.tolist() == [0, 0, 2, 2, 0, -2, 2 ** 19, -2 ** 19, 128, 128, -896] and n_out == 2
    assert (c == [2, 1]).all()
    r = E.integrate(geo, [pts - np.float32([0.1, 0.1, 0.0])], [0, 0], [pose, pose], p)      # an id twice counts twice
    cells = r["cells"]
    assert cells["count"][1, 2] == 22 and cells["count"].sum() == 22
    assert cells["zmin"][1, 2] == -2 ** 19 and cells["zmax"][1, 2] == 2 ** 19 and cells["sum"][1, 2] == 2 * sum(zq)
    assert cells["zmin"][0, 0] == E.I32_MAX and cells["zmax"][0, 0] == E.I32_MIN and cells["sum"][0, 0] == 0
    assert r["stats"] == dict(scans=2, points=26, points_marked=22, points_out_of_height=4, cells_new=1)
    again = E.integrate(geo, [pts], [0], [IDENT], p, cells)                                  # on top: no new cell there
    assert again["stats"]["cells_new"] == 0 and again["cells"]["count"][1, 2] == 33 and cells["count"][1, 2] == 22
    assert E.integrate(geo, [pts], [0], [[1e12, 0, 0, 1, 0, 0, 0]], p)["error"]              # the start cell beyond 2^30


def _cells_from_heights(z, count=3):
    """cells whose zmin is z (int quanta; None-like = E.I32_MAX means empty)"""
    z = np.asarray(z, np.int64)
    have = z != E.I32_MAX
    return dict(count=np.where(have, count, 0).astype(np.uint32), zmin=z.astype(np.int32),
                zmax=np.where(have, z + 5, E.I32_MIN).astype(np.int32), sum=np.where(have, count * z + 5, 0).astype(np.int64))


def test_plane_fit_is_exact_on_a_plane_and_nan_on_a_line():
    geo = E.geometry(0.5, 0.0, 0.0, 9, 7, 1.0)
    X, Y = np.meshgrid(np.arange(9), np.arange(7))
    cells = _cells_from_heights(12 * X - 5 * Y + 40)                                       # zmin = 12 i - 5 j + 40, in quanta
    for R in (1, 2, 4):
        d = E.derive(geo, cells, E.layer_params(1, R))
        assert (d["det"] > 0).all()
        want = (math.sqrt(12.0 * 12.0 + 5.0 * 5.0) * E.Q) / 0.5                             # = 13 / 128: exact
        assert (d["slope"] == want).all() and (d["rough"] == 0.0).all()                     # at the edges as in the middle
        assert (d["step"][1:-1, 1:-1] == 17 * E.Q).all() and (d["span"] == 5 * E.Q).all()
        assert d["step"][0, 0] == 12 * E.Q and d["step"][6, 0] == 17 * E.Q                  # a corner has three neighbours
    L = E.layers(geo, cells, E.layer_params(1, 1))
    assert L["min"][2, 3] == np.float32(1.0 + (36 - 10 + 40) * E.Q) and L["mean"][0, 0] == np.float32(1.0 + (125.0 * E.Q) / 3.0)
    # a single row, an isolated cell: det == 0, slope and roughness NaN, the step still defined
    z = np.full((7, 9), E.I32_MAX, np.int64)
    z[3, :] = 10 * np.arange(9)
    z[6, 0] = 77
    d = E.derive(geo, _cells_from_heights(z), E.layer_params(1, 2))
    assert (d["det"][d["valid"]] == 0).all() and np.isnan(d["slope"][3]).all() and np.isnan(d["rough"][6, 0])
    assert d["step"][3, 4] == 10 * E.Q and d["step"][6, 0] == 0.0
    L = E.layers(geo, _cells_from_heights(z), E.layer_params(1, 2))
    assert np.isnan(L["min"][0, 0]) and np.isnan(L["step"][0, 0]) and L["step"][3, 0] == np.float32(10 * E.Q)
    # min_points: a cell below it is invalid, and its neighbours do not see it
    d = E.derive(geo, cells, E.layer_params(4, 1))
    assert not d["valid"].any()


def test_cost_lands_on_every_branch():
    geo = E.geometry(1.0, 0.0, 0.0, 12, 5, 0.0)
    z = np.zeros((5, 12), np.int64)
    z[:, 4:] = 64          # a step of exactly 0.25 m between columns 3 and 4
    z[:, 8:] = 64 + 80     # and one of 0.3125 m between columns 7 and 8
    z[0, 0] = E.I32_MAX    # an empty cell
    cells = _cells_from_heights(z)
    cells["zmax"][2, 1] = 300                                                              # a span of 300 quanta: lethal by span alone
    cp = E.cost_params(max_slope=10.0, max_step=0.25, max_rough=10.0, max_span=1.0)
    cost, summary, seen = E.cost(geo, cells, E.layer_params(1, 1), cp)
    assert cost[0, 0] == E.UNKNOWN and cost[2, 1] == E.LETHAL and cost[2, 3] == 99 and cost[2, 4] == 99   # m == 1 exactly
    assert (cost[1:4, 7:9] == E.LETHAL).all() and cost[2, 10] == 0 and cost[2, 6] == 0
    assert seen["m_is_one"][2, 3] and seen["lethal_step"][2, 7] and seen["lethal_span"][2, 1] and not seen["lethal_slope"].any()
    assert summary == dict(cells_unknown=1, cells_lethal=int((cost == 100).sum()), cells_costed=int(((cost >= 0) & (cost < 100)).sum()))
    assert summary["cells_unknown"] + summary["cells_lethal"] + summary["cells_costed"] == 60
    # a slope beyond max_slope is lethal; rough beyond max_rough only saturates at 99
    X, Y = np.meshgrid(np.arange(12), np.arange(5))
    ramp = _cells_from_heights(100 * X)                                                    # 100 quanta per 1 m cell: slope 0.390625
    cost, _, seen = E.cost(geo, ramp, E.layer_params(1, 2), E.cost_params(0.3, 1.0, 1.0, 1.0))
    assert (cost == E.LETHAL).all() and seen["lethal_slope"].all() and not seen["lethal_step"].any()
    cost, _, seen = E.cost(geo, ramp, E.layer_params(1, 2), E.cost_params(0.78125, 1.0, 1.0, 1.0))
    assert (cost == 49).all()                                                              # floor(99 * 0.5)
    bumpy = _cells_from_heights(40 * ((X + Y) % 2))
    cost, _, seen = E.cost(geo, bumpy, E.layer_params(1, 2), E.cost_params(1.0, 1.0, 0.01, 1.0))
    assert seen["m_above_one"].all() and (cost == 99).all()


# ---- the scene -----------------------------------------------------------------------------------------------------------------
def test_scene_on_the_reference_alone():
    """Flat ground, a 10 degree ramp, a 0.15 m kerb, a wall and a beam above the band (tests/elevation_scene.py) through
    tests/elevation_ref.py.  Figures of this reference: ramp slope median 0.17813 against tan = 0.17633 (worst cell off by
    0.0109, 360 cells, none lethal, median cost 50); flat slope 0 and cost 0; kerb step median 0.1484 against 0.15 (worst off
    by 0.0016: the quantum is 0.0039; 58 cells, none lethal); wall cells lethal 100 % of 64; the beam leaves max = 0 under
    it and nothing lethal."""
    m = ES.measures()
    ref = ES.reference()
    out = os.path.join(ROOT, "profiles", "elevation_scene.json")
    try:
        with open(out, "w") as f:
            json.dump(dict(measures=m, stats=ref["stats"], summary=ref["summary"]), f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass  # (a read-only tree: the figures are printed all the same)
    print("elevation scene:", m)
    assert m["ramp_cells"] == 360 and m["kerb_cells"] == 58 and m["wall_cells"] == 64 and m["beam_cells"] == 16
    # the loose bounds, chosen from the figures above
    assert abs(m["ramp_slope_median"] - m["ramp_tan"]) <= 0.05 * m["ramp_tan"] and m["ramp_slope_worst"] <= 0.02
    assert m["ramp_lethal"] == 0.0 and 40 <= m["ramp_cost_median"] <= 60
    assert m["flat_slope_max"] <= 0.01 and m["flat_cost_max"] <= 2
    assert abs(m["kerb_step_median"] - ES.KERB_H) <= E.Q and m["kerb_step_worst"] <= E.Q and m["kerb_lethal"] == 0.0
    assert m["wall_lethal"] >= 0.95
    assert m["beam_max"] <= 0.1 and m["beam_lethal"] == 0.0
    # the recorded figures
    assert round(m["ramp_slope_median"], 5) == 0.17813 and round(m["ramp_slope_worst"], 4) == 0.0109
    assert m["ramp_cost_median"] == 50.0 and m["flat_slope_max"] == 0.0 and m["flat_cost_max"] == 0
    assert m["kerb_step_median"] == 0.1484375 and round(m["kerb_step_worst"], 4) == 0.0016
    assert m["wall_lethal"] == 1.0 and m["beam_max"] == 0.0
    assert ref["stats"] == dict(scans=6, points=175929, points_marked=155450, points_out_of_height=0, cells_new=4288)
    assert ref["summary"] == dict(cells_unknown=324, cells_lethal=93, cells_costed=4191)


# ---- declarations and refusals -----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"elevation grid", text) and re.search(r"#define LOM_ELEV_QUANTUM_LOG2 \(-8\)", text)
    assert re.search(r"LOM_ELEV_OPT_TEST_WAVE_MERGE\s*=\s*1", text)
    assert lom.capi.lib().lom_abi_version() == 2
    assert (lom.capi.ELEV_COST_UNKNOWN, lom.capi.ELEV_COST_LETHAL) == (E.UNKNOWN, E.LETHAL)
    assert 2.0 ** lom.capi.ELEV_QUANTUM_LOG2 == E.Q
    sizes = dict(ElevationGeometry=24, ElevationPointParams=16, ElevationLayerParams=8, ElevationCostParams=16, ElevationStats=40,
                 ElevationSummary=24)
    for name, size in sizes.items():
        assert C.sizeof(getattr(lom.capi, name)) == size, name
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for name in ("integrate", "integrateCloud", "cells", "layers", "cost", "clear", "elevationScan"):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
    assert re.search(r"class ElevationGrid", mirror)
    for name in ("integrate", "integrateCloud", "cells", "layers", "cost", "clear"):
        assert hasattr(lom.ElevationGrid, name), name
    assert hasattr(lom.LidarOdometry, "elevationScan")


def test_bad_arguments_are_refused_without_a_device(lom):
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    h = C.c_void_p()
    good = dict(resolution=0.25, origin_x=0.0, origin_y=0.0, width=10, height=10, z_ref=0.0)
    for change in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=np.nan), dict(resolution=np.inf),
                   dict(origin_x=np.nan), dict(origin_y=np.inf), dict(width=0), dict(height=0), dict(width=8193),
                   dict(height=8193), dict(z_ref=np.nan), dict(z_ref=-np.inf)):
        geo = lom.capi.ElevationGeometry(**dict(good, **change))
        assert L.lom_elevation_create(C.byref(geo), 0, C.byref(h)) == ERR_ARG, change
        assert b"geometry" in L.lom_elevation_last_error(None)
    assert L.lom_elevation_create(None, 0, C.byref(h)) == ERR_ARG
    assert L.lom_elevation_create(C.byref(lom.capi.ElevationGeometry(**good)), 0, None) == ERR_ARG
    st = lom.capi.ElevationStats()
    st.scans = 7
    prm = lom.elevationPointParams(ES.POINTS)
    lp, cp = lom.elevationLayerParams(ES.LAYER), lom.elevationCostParams(ES.COST)
    assert L.lom_elevation_integrate(None, None, None, None, 0, C.byref(prm), C.byref(st)) == ERR_ARG and st.scans == 0
    assert L.lom_elevation_integrate_cloud(None, None, 0, 12, None, C.byref(prm), None) == ERR_ARG
    assert L.lom_elevation_integrate_cloud_device(None, None, 0, 12, None, C.byref(prm), None, None) == ERR_ARG
    assert L.lom_elevation_cells(None, None, None, None, None, 0) == ERR_ARG
    assert L.lom_elevation_layers(None, C.byref(lp), None, None, None, None, None, None, 0) == ERR_ARG
    sm = lom.capi.ElevationSummary()
    sm.cells_lethal = 5
    assert L.lom_elevation_cost(None, C.byref(lp), C.byref(cp), None, 0, C.byref(sm)) == ERR_ARG and sm.cells_lethal == 0
    assert L.lom_elevation_cost_device(None, C.byref(lp), C.byref(cp), C.byref(h)) == ERR_ARG
    assert L.lom_elevation_clear(None) == ERR_ARG and L.lom_elevation_device(None) == ERR_ARG
    assert L.lom_elevation_get_geometry(None, None) == ERR_ARG and L.lom_elevation_wait_event(None, None) == ERR_ARG
    assert L.lom_elevation_set_option(None, 1, 1) == ERR_ARG and L.lom_elevation_stream(None) is None
    st.scans = 7
    assert L.lom_odometry_elevation_scan(None, None, C.byref(prm), C.byref(st)) == ERR_ARG and st.scans == 0
    L.lom_elevation_destroy(None)
    with pytest.raises(TypeError):
        lom.elevationPointParams(dict(z_lo=-1.0))  # no defaults: all four fields or none
    assert lom.elevationLayerParams((3, 2)).window == 2 and lom.elevationCostParams((1, 2, 3, 4)).max_rough == 3.0
