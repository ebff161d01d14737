"""Occupancy grid, the parts that need no GPU: the walk of the reference (tests/occupancy_ref.py) against brute-force
geometry, the hit / band / range rules by hand, the corridor scene on the reference alone, the declarations and the
refusals that touch no device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import occupancy_ref as O
from tests import occupancy_scene as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_occupancy_create", "lom_occupancy_destroy", "lom_occupancy_last_error", "lom_occupancy_clear",
               "lom_occupancy_get_geometry", "lom_occupancy_stream", "lom_occupancy_device", "lom_occupancy_wait_event",
               "lom_occupancy_set_option", "lom_occupancy_integrate", "lom_occupancy_integrate_cloud",
               "lom_occupancy_integrate_cloud_device", "lom_occupancy_counts", "lom_occupancy_classify",
               "lom_occupancy_classify_device", "lom_odometry_archive_deskewed", "lom_odometry_occupancy_scan"]
IDENT = [0, 0, 0, 1, 0, 0, 0]


# ---- the walk against geometry ---------------------------------------------------------------------------------------------
def segment_range_in_box(a, d, lo, hi):
    """[t0, t1] of the parameters t in [0, 1] with a + t d inside the closed box [lo, hi] (2-D), or None"""
    t0, t1 = 0.0, 1.0
    for k in range(2):
        if d[k] == 0.0:
            if a[k] < lo[k] or a[k] > hi[k]:
                return None
        else:
            u, v = (lo[k] - a[k]) / d[k], (hi[k] - a[k]) / d[k]
            t0, t1 = max(t0, min(u, v)), min(t1, max(u, v))
    return (t0, t1) if t0 <= t1 else None


def check_walk_against_geometry(geo, origin, pts, p, eps=1e-9):
    r = float(np.float32(geo["resolution"]))
    O2, c0, ok = O.start_cell(geo, origin)
    assert ok
    w = O.walk(geo, origin, pts, p)
    R = O.rays(geo, origin, pts, p)
    n_walked = 0
    for i in range(len(pts)):
        got = [tuple(c) for c in w["cell"][w["ray"] == i].tolist()]
        if not R["walked"][i]:
            assert got == []
            continue
        n_walked += 1
        assert len(set(got)) == len(got), i                                   # no cell twice
        d = R["D"][i][:2] * R["t_end"][i]                                     # the walked part of the ray, in 2-D
        for c in got:                                                        # every visited cell's closed box meets it
            lo = np.array(c, np.float64) * r
            assert segment_range_in_box(O2, d, lo - eps, lo + r + eps) is not None, (i, c)
        reach = int(np.ceil(np.abs(d).max() / r)) + 2
        visited = set(got)
        for cx in range(int(c0[0]) - reach, int(c0[0]) + reach + 1):          # every cell whose interior meets it is visited
            for cy in range(int(c0[1]) - reach, int(c0[1]) + reach + 1):
                if (cx, cy) in visited:
                    continue
                lo = np.array([cx, cy], np.float64) * r
                rng = segment_range_in_box(O2, d, lo + eps, lo + r - eps)
                assert rng is None, (i, (cx, cy))
    return n_walked


@pytest.mark.parametrize("seed,res", [(1, 0.25), (2, 0.1), (3, 0.5)])
def test_walk_visits_the_cells_the_segment_meets(seed, res):
    """1,000 random segments per case (3,000 in all): origins inside a cell, on a plane and on a corner; zero components;
    exact diagonals"""
    rng = np.random.default_rng(seed)
    geo = O.geometry(res, -3.0, -2.0, 64, 48)
    p = O.ray_params(-1.0, 1.5, 0.25 * res, 1.5 * res, 12 * res)
    total = 0
    for kind in range(4):
        cell = np.array([11, 9], np.float64)
        frac = rng.uniform(0.1, 0.9, 2)
        if kind == 1:
            frac[0] = 0.0                                  # on a plane
        if kind == 2:
            frac[:] = 0.0                                  # on a corner
        o2 = (cell + frac) * res                            # (binary fractions of res where frac is 0: exactly on the plane)
        origin = np.array([o2[0] - 3.0, o2[1] - 2.0, 0.3], np.float32)
        n = 250
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        d *= rng.uniform(0.5 * res, 16 * res, (n, 1))
        d[:20, 0] = 0.0                                     # zero components
        d[20:40, 1] = 0.0
        d[40:50, 2] = 0.0
        k = rng.integers(1, 12, 30) * res
        d[50:80, 0], d[50:80, 1] = k * rng.choice([-1, 1], 30), k * rng.choice([-1, 1], 30)   # exact diagonals
        pts = (origin.astype(np.float64) + d).astype(np.float32)
        total += check_walk_against_geometry(geo, origin, pts, p)
    assert total > 600


# ---- hit, band and range by hand ---------------------------------------------------------------------------------------------
def test_hit_band_and_range_rules():
    geo = O.geometry(0.5, 0.0, 0.0, 20, 10)
    p = O.ray_params(z_lo=-1.0, z_hi=0.5, margin=0.25, min_range=1.0, max_range=4.0)
    o = np.array([2.25, 2.25, 1.0], np.float32)
    nan, inf = np.nan, np.inf
    pts = np.array([
        [5.25, 2.25, 1.0],     # 0 level: L = 3, walked to 2.75 m, hit in cell (10, 4)
        [5.25, 2.25, 1.5],     # 1 Dz = z_hi exactly: still a hit
        [5.25, 2.25, 1.75],    # 2 above the band: no hit, walked to where it leaves the band (t = 2/3)
        [5.25, 2.25, 0.0],     # 3 Dz = z_lo exactly: a hit
        [5.25, 2.25, -0.25],   # 4 below the band: no hit
        [3.25, 2.25, 1.0],     # 5 L = min_range exactly: walked and hit
        [3.0, 2.25, 1.0],      # 6 L < min_range: neither
        [6.25, 2.25, 1.0],     # 7 L = max_range exactly: hit, walked to 3.75 m
        [6.75, 2.25, 1.0],     # 8 beyond max_range: no hit, walked to 3.75 m
        [2.25, 2.25, 1.0],     # 9 zero length: neither
        [nan, 2.25, 1.0],      # 10
        [inf, 2.25, 1.0],      # 11
        [2.25, -0.75, 1.0],    # 12 endpoint outside the grid: no hit, the walk leaves the grid
        [2.25, 2.25, -inf],    # 13
    ], np.float32)
    R = O.rays(geo, o, pts, p)
    assert R["hit"].tolist() == [True, True, False, True, False, True, False, True, False, False, False, False, False, False]
    assert R["walked"].tolist() == [True, True, True, True, True, True, False, True, True, False, False, False, True, False]
    assert R["hit_cell"][0].tolist() == [10, 4] and R["hit_cell"][7].tolist() == [12, 4]
    assert R["t_end"][0] == 2.75 / 3.0 and R["t_end"][2] == 0.5 / 0.75 and R["t_end"][7] == 3.75 / 4.0
    w = O.walk(geo, o, pts, p)
    last = {i: w["cell"][w["ray"] == i][-1].tolist() for i in (0, 2, 5, 7, 8, 12)}
    # x = 2.25 + 2.75 = 5.0: t_a <= t_end steps INTO cell 10; 2.25 + 2 = 4.25: cell 8; 3.0: cell 6; 6.0: cell 12;
    # y = 2.25 - 2.75 = -0.5, on the plane again: into cell -2
    assert last == {0: [10, 4], 2: [8, 4], 5: [6, 4], 7: [12, 4], 8: [12, 4], 12: [4, -2]}
    b = O.scan_bits(geo, np.r_[o.astype(np.float64), 1, 0, 0, 0], pts - o, p)
    assert b["walked"] == 9 and b["marked"] == 5 and b["hit"].sum() == 3 and not b["passed"][:, 13:].any()
    # the walk of ray 12 counts its two cells outside the grid as visited, and marks nothing there
    assert b["visited"] == len(w["ray"]) and (w["cell"][:, 1] < 0).sum() == 2


def test_votes_count_scans_and_accumulate():
    geo = O.geometry(0.5, 0.0, 0.0, 12, 4)
    p = O.ray_params(-1.0, 1.0, 0.0, 0.5, 10.0)
    through = np.array([[4.0, 0.02 * i, 0.0] for i in range(5)], np.float32)   # five rays through cells 0 .. 8
    onto = np.array([[2.0, 0.0, 0.0]], np.float32)                              # one point into cell (4, 2)
    pose = [0.25, 1.25, 0.0, 1, 0, 0, 0]
    r = O.integrate(geo, [through, onto], [0, 1], [pose, pose], p)
    assert r["seen"][2].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert r["free"][2].tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 0, 0, 0, 0]       # scans, not rays; a hit cell is not free
    assert r["stats"] == dict(scans=2, rays_walked=6, rays_skipped=0, endpoints_marked=6, cells_visited=5 * 9 + 5)
    r2 = O.integrate(geo, [through, onto], [0, 0], [pose, pose], p, free=r["free"], seen=r["seen"])   # an id twice, on top
    assert r2["free"][2, 0] == 4 and r2["seen"][2, 8] == 3 and r2["seen"][2, 4] == 1
    cls, summary = O.classify(r2["free"], r2["seen"], O.rule(2, 2, 1))
    assert cls[2].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 100, -1, -1, -1]          # cell 4: free 3 >= 2 * seen 1
    assert summary == dict(cells_free=8, cells_occupied=1, cells_unknown=39)
    assert O.integrate(geo, [onto], [0], [[1e12, 0, 0, 1, 0, 0, 0]], p)["error"]    # the start cell beyond 2^30
    assert not O.integrate(geo, [onto], [0], [[1e8, 0, 0, 1, 0, 0, 0]], p)["error"]


# ---- the corridor scene ------------------------------------------------------------------------------------------------------
def test_corridor_scene_on_the_reference_alone():
    """The scene, grid, parameters and masks of tests/occupancy_scene.py through tests/occupancy_ref.py; the conditions are
    the feature's issue's.  Figures of this reference, with / without the mover: swept cells with seen >= 1 14.7 % / 0 %,
    swept FREE 100 % / 100 %, corridor FREE 99.74 %, corridor OCCUPIED 0.085 %, wall columns 100 % and 97.2 % (312 swept
    cells, 16,560 corridor cells)."""
    m1, m0 = OS.measures(True), OS.measures(False)
    out = os.path.join(ROOT, "profiles", "occupancy_scene.json")
    try:
        with open(out, "w") as f:
            json.dump(dict(with_mover=m1, without_mover=m0, stats_with_mover=OS.reference(True)["stats"]), f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass  # (a read-only tree: the figures are printed all the same)
    print("occupancy scene:", m1, m0)
    assert m1["swept_cells"] == 312 and m1["corridor_cells"] == 16560
    assert m1["swept_seen"] >= 0.10        # the mover leaves a trace for the rule to remove
    assert m1["swept_free"] >= 0.95
    assert m0["swept_seen"] == 0.0
    for m in (m1, m0):
        assert m["corridor_free"] >= 0.99
        assert m["corridor_occupied"] <= 0.005
        assert m["wall_lo"] >= 0.90 and m["wall_hi"] >= 0.90
    # the recorded figures
    assert round(m1["swept_seen"], 3) == 0.147 and m1["swept_free"] == 1.0 and m0["swept_free"] == 1.0
    for m in (m1, m0):
        assert round(m["corridor_free"], 4) == 0.9974 and round(m["corridor_occupied"], 5) == 0.00085
        assert m["wall_lo"] == 1.0 and round(m["wall_hi"], 3) == 0.972


# ---- declarations and refusals -----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    for name in lom.capi.EXPORTED_BY_TYPE_POINTS:   # declared through their types, as lom_graph_pose_rotation_matrix is
        assert re.search(r"_fn %s;" % name, text) and getattr(lom.capi.lib(), name).argtypes is not None, name
    assert lom.capi.EXPORTED_BY_TYPE_POINTS == ["lom_archive_add_points", "lom_archive_add_points_device"]
    assert re.search(r"occupancy grid", text) and re.search(r"LOM_OCC_OPT_TEST_WINDOW\s*=\s*2", text)
    assert (lom.capi.OCC_FREE, lom.capi.OCC_OCCUPIED, lom.capi.OCC_UNKNOWN) == (O.FREE, O.OCCUPIED, O.UNKNOWN)
    assert C.sizeof(lom.capi.OccupancyGeometry) == 20 and C.sizeof(lom.capi.OccupancyStats) == 40
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for name in ("integrate", "integrateCloud", "counts", "classify", "clear", "occupancyScan", "archiveDeskewed", "addPoints"):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
    assert re.search(r"class OccupancyGrid", mirror)
    for name in ("integrate", "integrateCloud", "counts", "classify", "clear"):
        assert hasattr(lom.OccupancyGrid, name), name
    assert hasattr(lom.LidarOdometry, "occupancyScan") and hasattr(lom.LidarOdometry, "archiveDeskewed")
    assert hasattr(lom.ScanArchive, "addPoints")


def test_bad_arguments_are_refused_without_a_device(lom):
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    h = C.c_void_p()
    good = dict(resolution=0.25, origin_x=0.0, origin_y=0.0, width=10, height=10)
    for change in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=np.nan), dict(resolution=np.inf),
                   dict(origin_x=np.nan), dict(origin_y=np.inf), dict(width=0), dict(height=0), dict(width=16385),
                   dict(height=16385)):
        geo = lom.capi.OccupancyGeometry(**dict(good, **change))
        assert L.lom_occupancy_create(C.byref(geo), 0, C.byref(h)) == ERR_ARG, change
        assert b"geometry" in L.lom_occupancy_last_error(None)
    assert L.lom_occupancy_create(None, 0, C.byref(h)) == ERR_ARG
    assert L.lom_occupancy_create(C.byref(lom.capi.OccupancyGeometry(**good)), 0, None) == ERR_ARG
    st = lom.capi.OccupancyStats()
    st.scans = 7
    prm = lom.occupancyRayParams(OS.PARAMS)
    assert L.lom_occupancy_integrate(None, None, None, None, 0, C.byref(prm), C.byref(st)) == ERR_ARG and st.scans == 0
    assert L.lom_occupancy_integrate_cloud(None, None, 0, 12, None, C.byref(prm), None) == ERR_ARG
    assert L.lom_occupancy_integrate_cloud_device(None, None, 0, 12, None, C.byref(prm), None, None) == ERR_ARG
    assert L.lom_occupancy_counts(None, None, None, 0) == ERR_ARG
    assert L.lom_occupancy_classify(None, None, None, 0, None) == ERR_ARG
    assert L.lom_occupancy_clear(None) == ERR_ARG and L.lom_occupancy_device(None) == ERR_ARG
    assert L.lom_occupancy_set_option(None, 1, 1) == ERR_ARG
    assert L.lom_archive_add_points(None, None, 0, 12) == ERR_ARG
    assert L.lom_odometry_occupancy_scan(None, None, C.byref(prm), C.byref(st)) == ERR_ARG
    assert L.lom_odometry_archive_deskewed(None, None, None) == ERR_ARG
    with pytest.raises(TypeError):
        lom.occupancyRayParams(dict(margin=0.3))  # no defaults: all five fields or none
    assert lom.occupancyRule((3, 2, 1)).free_per_seen == 2
