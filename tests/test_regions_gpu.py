"""The region grid on the device against tests/regions_ref.py: the labels as bytes, the summary, the records as bytes, the
list under each rank, both goal kinds and the query -- all exactly equal, under every setting of the test switches.  The
reference of a case is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import occupancy_ref as O
from tests import regions_ref as R
from tests import regions_scenes as RS

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)
SHAPES = [(1, 1), (1, 70), (70, 1), (32, 32), (33, 31), (64, 32), (65, 33), (128, 64), (129, 65)]
RANGES = [(0, 98), (100, 100), (-1, -1)]
# tile rows, no tiles, no wave merge
SWITCHES = [(rows, no_tiles, no_merge) for rows in (1, 8, 32) for no_tiles in (0, 1) for no_merge in (0, 1)]
REFS = {}


def geo_of(w, h):
    return N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)


def reference(key, plane, p, cost=None, potential=None, max_regions=R.MAX_REGIONS_DEFAULT):
    """the reference's extract of a case, once"""
    if key not in REFS:
        REFS[key] = R.extract(plane, p, cost, potential, max_regions)
    return REFS[key]


def set_switches(lom, dev, rows, no_tiles, no_merge):
    dev.setOption(lom.capi.REGIONS_OPT_TEST_TILE_ROWS, rows)
    dev.setOption(lom.capi.REGIONS_OPT_TEST_NO_TILES, no_tiles)
    dev.setOption(lom.capi.REGIONS_OPT_TEST_NO_WAVE_MERGE, no_merge)


def check_extract(dev, ref, plane, p, cost=None, potential=None, what=None):
    """one extract against the reference: summary, labels, records (the list under the label rank with min_cells 1 is every
    record) or the list, and both goal kinds"""
    summary = dev.extract(plane, R.as_tuple(p), cost, potential)
    assert summary == ref["summary"], (what, summary, ref["summary"])
    got = dev.labels()
    assert got.tobytes() == ref["labels"].tobytes(), (what, np.argwhere(got != ref["labels"])[:10])
    lst = dev.list()
    if p["rank"] == R.RANK_LABEL and p["min_cells"] == 1:
        assert lst.tobytes() == ref["records"].tobytes(), (what, lst[:4], ref["records"][:4])
    want = R.sort_list(ref["records"], p["min_cells"], p["rank"])
    assert lst.tobytes() == want.tobytes(), what
    for which in (R.GOAL_CENTRE, R.GOAL_ENTRY):
        assert np.array_equal(dev.goals(which), R.goals(want, which)), (what, which)
    st = dev.stats()
    assert st["waits"] == 1 and 8 <= st["launches"] <= 11


def potential_plane(rng, w, h):
    """a u32 plane in lom_navfield_potential's form: few distinct values, so the least P ties, and some cells unreached"""
    pot = rng.integers(0, 40, (h, w)).astype(np.uint32) * 250
    pot[rng.random((h, w)) < 0.1] = N.UNREACHED
    return pot


def cases_of(w, h):
    """name -> (plane, params, cost, potential, max_regions) for a shape"""
    rng = np.random.default_rng(1000 * w + h)
    planes = {"random": S.random_plane(rng, w, h), "serpentine": S.serpentine(w, h), "spiral": S.spiral(w, h),
              "diagonal_gaps": S.diagonal_gaps(w, h), "pocket": S.pocket(w, h)}
    out = {}
    for conn in (0, R.CONNECT_4):
        for name, plane in planes.items():
            for lo, hi in RANGES:
                out[(name, lo, hi, conn)] = (plane, R.params(R.BYTES, lo, hi, flags=conn), None, None, None)
        by = R.params(R.BYTES, 100, 100, flags=conn)
        out[("full", conn)] = (RS.full(w, h), by, None, None, None)
        out[("empty", conn)] = (RS.empty(w, h), by, None, None, None)
        out[("dots", conn)] = (RS.dots(w, h), by, None, None, None)
        out[("dots_3", conn)] = (RS.dots(w, h), by, None, None, 3)
        out[("staircase", conn)] = (RS.staircase(w, h), by, None, None, None)
    occ = RS.frontier_plane(w, h)
    cost, pot = S.random_plane(rng, w, h, obstacles=0.1, unknown=0.05), potential_plane(rng, w, h)
    for with_planes in (False, True):
        for flags in (0, R.NEIGHBOURS_8, R.EDGE_UNKNOWN, R.NEIGHBOURS_8 | R.EDGE_UNKNOWN, R.CONNECT_4 | R.EDGE_UNKNOWN):
            p = R.params(R.FRONTIER, max_cost=60, flags=flags)
            out[("frontier", with_planes, flags)] = (occ, p, cost if with_planes else None, pot if with_planes else None, None)
    return out


# ---- 1: shapes x scenes x switches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_scenes_and_switches(lom, w, h):
    rng = np.random.default_rng(w + 7 * h)
    dev = lom.RegionGrid(RES, ORIGIN, w, h)
    geo = geo_of(w, h)
    assert (dev.labels() == R.NONE).all() and len(dev.list()) == 0 and len(dev.goals()) == 0      # after create
    for name, (plane, p, cost, pot, cap) in cases_of(w, h).items():
        ref = reference((w, h, name), plane, p, cost, pot, cap or R.MAX_REGIONS_DEFAULT)
        assert not ref["error"]
        dev.setOption(lom.capi.REGIONS_OPT_MAX_REGIONS, cap or 0)
        for rows, no_tiles, no_merge in SWITCHES:
            set_switches(lom, dev, rows, no_tiles, no_merge)
            check_extract(dev, ref, plane, p, cost, pot, what=(name, rows, no_tiles, no_merge))
        # the list under the other ranks and a larger min_cells, and the query, on the default switches
        set_switches(lom, dev, 0, 0, 0)
        for rank in (R.RANK_CELLS, R.RANK_POTENTIAL):
            if rank == R.RANK_POTENTIAL and pot is None:
                continue
            for min_cells in (1, 3):
                q = dict(p, rank=rank, min_cells=min_cells)
                want = dict(ref, summary=dict(ref["summary"], regions_listed=int((ref["records"]["cells"] >= min_cells).sum())))
                check_extract(dev, want, plane, q, cost, pot, what=(name, rank, min_cells))
        xy = np.concatenate([rng.uniform(ORIGIN[0] - 1.0, ORIGIN[0] + w * RES + 1.0, (50, 1)),
                             rng.uniform(ORIGIN[1] - 1.0, ORIGIN[1] + h * RES + 1.0, (50, 1))], axis=1).astype(np.float32)
        assert np.array_equal(dev.query(xy), R.query(geo, ref["labels"], xy)), name
    # what the scenes are for, on the reference
    if (w, h) == (129, 65):
        assert REFS[(w, h, ("full", 0))]["summary"]["largest_cells"] == w * h
        assert REFS[(w, h, ("dots", 0))]["summary"]["regions"] == 65 * 33
        assert REFS[(w, h, ("dots_3", R.CONNECT_4))]["summary"]["regions_recorded"] == 3
        assert REFS[(w, h, ("staircase", 0))]["summary"]["regions"] == 1 and REFS[(w, h, ("staircase", R.CONNECT_4))]["summary"]["regions"] == 65
        assert REFS[(w, h, ("serpentine", 0, 98, 0))]["summary"]["largest_cells"] == 4289
        assert REFS[(w, h, ("spiral", 0, 98, R.CONNECT_4))]["summary"]["largest_cells"] == 4290
        assert REFS[(w, h, ("frontier", False, 0))]["summary"]["regions"] > 30
        assert 0 < REFS[(w, h, ("frontier", True, 0))]["summary"]["cells_member"] < REFS[(w, h, ("frontier", False, 0))]["summary"]["cells_member"]
        set_switches(lom, dev, 32, 0, 0)
        dev.extract(RS.full(w, h), R.as_tuple(R.params(R.BYTES, 100, 100)))
        assert dev.stats()["tiles"] == 9                              # 3 x 3 tiles, a one-cell tile column and tile row


def test_query_at_cell_borders(lom):
    w, h = 65, 33
    plane = RS.frontier_plane(w, h)
    p = R.params(R.FRONTIER, flags=R.EDGE_UNKNOWN)
    ref = reference("query", plane, p)
    dev = lom.RegionGrid(RES, ORIGIN, w, h)
    check_extract(dev, ref, plane, p)
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(4)
    xy = np.array([[-3.0, 2.0], [-2.75, 2.25], [-2.7500002, 2.2499998], [13.249999, 10.249999], [13.25, 5.0], [5.0, 10.25],
                   [-3.0000002, 5.0], [nan, 5.0], [5.0, nan], [inf, 5.0], [5.0, -inf], [1e30, -1e30]], np.float32)
    xy = np.concatenate([xy, rng.uniform(-5, 15, (300, 2)).astype(np.float32)])
    got, want = dev.query(xy), R.query(geo_of(w, h), ref["labels"], xy)
    assert np.array_equal(got, want) and (want[4:12] == R.NONE).all() and (want != R.NONE).sum() > 20
    assert len(dev.query(np.zeros((0, 2), np.float32))) == 0
    assert lom.capi.lib().lom_regions_query(dev.handle, None, 3, None) == lom.capi.ERR_ARG


# ---- 2: purity and refusals ----------------------------------------------------------------------------------------------------
def test_two_runs_agree_and_a_refused_call_changes_nothing(lom):
    w, h = 129, 65
    rng = np.random.default_rng(30)
    plane, cost, pot = RS.frontier_plane(w, h), S.random_plane(rng, w, h, obstacles=0.1), potential_plane(rng, w, h)
    p = R.params(R.FRONTIER, max_cost=70, min_cells=2, rank=R.RANK_POTENTIAL, flags=R.NEIGHBOURS_8)
    dev = lom.RegionGrid(RES, ORIGIN, w, h)
    first = dev.extract(plane, R.as_tuple(p), cost, pot)
    labels, lst, goals = dev.labels(), dev.list(), dev.goals(R.GOAL_ENTRY)
    dev.extract(S.serpentine(w, h), R.as_tuple(R.params(R.BYTES, 0, 98)))
    assert dev.labels().tobytes() != labels.tobytes()
    assert dev.extract(plane, R.as_tuple(p), cost, pot) == first
    assert dev.labels().tobytes() == labels.tobytes() and dev.list().tobytes() == lst.tobytes()
    ref = reference("purity", plane, p, cost, pot)
    assert first == ref["summary"] and labels.tobytes() == ref["labels"].tobytes() and lst.tobytes() == ref["list"].tobytes()
    assert len(lst) > 3 and (np.diff(lst["entry_potential"].astype(np.int64)) >= 0).all()
    # refused: bad values, unknown flag bits, a rank by potential without one, no plane; the summary is zeroed
    L = lom.capi.lib()
    sm = lom.capi.RegionsSummary()
    other = S.spiral(w, h)
    bad_params = [(2, 0, 0, 99, 1, 0, 0), (-1, 0, 0, 99, 1, 0, 0), (0, 5, 4, 99, 1, 0, 0), (1, 0, 0, 100, 1, 0, 0), (1, 0, 0, -1, 1, 0, 0),
                  (1, 0, 0, 99, 0, 0, 0), (1, 0, 0, 99, 1, 3, 0), (1, 0, 0, 99, 1, -1, 0), (1, 0, 0, 99, 1, 0, 8), (1, 0, 0, 99, 1, 0, 1 << 31)]
    for bad in bad_params:
        sm.cells_member = 9
        prm = lom.regionsParams(bad)
        assert L.lom_regions_extract(dev.handle, other.ctypes.data, None, pot.ctypes.data, C.byref(prm), C.byref(sm)) == lom.capi.ERR_ARG, bad
        assert sm.asdict() == dict.fromkeys(R.SUMMARY_KEYS, 0) and L.lom_regions_last_error(dev.handle)
    by_potential = lom.regionsParams((1, 0, 0, 99, 1, R.RANK_POTENTIAL, 0))
    good = lom.regionsParams((1, 0, 0, 99, 1, 0, 0))
    sm.cells_member = 9
    assert L.lom_regions_extract(dev.handle, other.ctypes.data, None, None, C.byref(by_potential), C.byref(sm)) == lom.capi.ERR_ARG
    assert sm.cells_member == 0
    assert L.lom_regions_extract(dev.handle, None, None, None, C.byref(good), C.byref(sm)) == lom.capi.ERR_ARG
    assert L.lom_regions_extract(dev.handle, other.ctypes.data, None, None, None, C.byref(sm)) == lom.capi.ERR_ARG
    assert L.lom_regions_extract_device(dev.handle, None, None, None, None, C.byref(good), C.byref(sm)) == lom.capi.ERR_ARG
    assert L.lom_regions_goals(dev.handle, 2, None, 0, None) == lom.capi.ERR_ARG
    with pytest.raises(ValueError):
        dev.extract(plane[:-1], R.as_tuple(p))
    for option, bad in ((lom.capi.REGIONS_OPT_MAX_REGIONS, (1 << 26) + 1), (lom.capi.REGIONS_OPT_TEST_TILE_ROWS, 16),
                        (lom.capi.REGIONS_OPT_TEST_NO_TILES, 2), (lom.capi.REGIONS_OPT_TEST_NO_WAVE_MERGE, 2), (77, 0)):
        with pytest.raises(lom.LomError):
            dev.setOption(option, bad)
    # nothing changed
    assert dev.labels().tobytes() == labels.tobytes() and dev.list().tobytes() == lst.tobytes()
    assert np.array_equal(dev.goals(R.GOAL_ENTRY), goals)
    assert dev.geometry() == dict(resolution=RES, origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=w, height=h)
    assert L.lom_regions_device(dev.handle) == 0 and L.lom_regions_stream(dev.handle)
    # partial outputs
    few = np.full(50, 7, np.uint32)
    assert L.lom_regions_labels(dev.handle, few.ctypes.data, 20) == 0
    assert np.array_equal(few[:20], labels.ravel()[:20]) and (few[20:] == 7).all()
    two, n = np.zeros(2, lom.capi.REGIONS_RECORD), C.c_size_t()
    assert L.lom_regions_list(dev.handle, two.ctypes.data, 2, C.byref(n)) == 0 and n.value == len(lst) and two.tobytes() == lst[:2].tobytes()
    dev.clear()
    assert (dev.labels() == R.NONE).all() and len(dev.list()) == 0 and len(dev.goals()) == 0
    with pytest.raises(lom.LomError) as e:
        lom.RegionGrid(0.5, (0, 0), 10, 8193)
    assert e.value.code == lom.capi.ERR_ARG


# ---- 3: with the other grids -----------------------------------------------------------------------------------------------------
def test_extract_from_grids_and_goals_into_the_navfield(lom):
    from tests.test_occupancy_gpu import archive_of
    from tests.test_vote_gpu import pose_in_room, room_scan

    rng = np.random.default_rng(92)
    res, org, w, h = 0.1, (-5.0, -4.0), 100, 80
    poses = np.stack([pose_in_room(rng, turn=0.6) for _ in range(3)])
    scans = [room_scan(rng, 4000, poses[k])[0] for k in range(3)]
    rays = O.ray_params(z_lo=-2.5, z_hi=2.5, margin=0.05, min_range=1.0, max_range=3.0)
    rule = O.rule(1, 1, 1)
    occ = lom.OccupancyGrid(res, org, w, h)
    occ.integrate(archive_of(lom, scans), np.arange(3), poses, rays)
    occ_plane = occ.classify(rule)[0]
    assert (occ_plane == 0).sum() > 500 and (occ_plane == -1).sum() > 500
    clear = lom.ClearanceGrid(res, org, w, h)
    clear.update(occ_plane, None, K.params(0.5, 0.15, 2.0))
    cost = clear.cost()[0]
    nav = lom.NavField(res, org, w, h)
    np_params = (50, 3, 400, 98, 0)
    robot = np.argwhere(cost == 0)[:1, ::-1].astype(np.int32)
    assert len(robot) == 1
    assert nav.solveFromClearance(clear, np_params, robot)["cells_reached"] > 500
    pot = nav.potential()
    dev, host = lom.RegionGrid(res, org, w, h), lom.RegionGrid(res, org, w, h)
    for c, f, rank in ((clear, nav, R.RANK_POTENTIAL), (clear, None, R.RANK_CELLS), (None, nav, R.RANK_POTENTIAL), (None, None, R.RANK_LABEL)):
        p = R.params(R.FRONTIER, max_cost=98, min_cells=2, rank=rank)
        got = dev.extractFromGrids(occ, rule, c, f, R.as_tuple(p))
        cost_in, pot_in = (None if c is None else cost), (None if f is None else pot)
        assert got == host.extract(occ_plane, R.as_tuple(p), cost_in, pot_in)
        assert dev.labels().tobytes() == host.labels().tobytes() and dev.list().tobytes() == host.list().tobytes()
        ref = reference(("grids", c is None, f is None), occ_plane, p, cost_in, pot_in)
        assert got == ref["summary"] and dev.labels().tobytes() == ref["labels"].tobytes() and dev.list().tobytes() == ref["list"].tobytes()
    assert REFS[("grids", False, False)]["summary"]["regions_listed"] >= 1
    # the producers go on: the same planes again
    assert np.array_equal(occ.classify(rule)[0], occ_plane) and np.array_equal(clear.cost()[0], cost) and np.array_equal(nav.potential(), pot)
    # the loop closes: the regions' goals into the navigation field
    dev.extractFromGrids(occ, rule, clear, nav, R.as_tuple(R.params(R.FRONTIER, max_cost=98, min_cells=2, rank=R.RANK_POTENTIAL)))
    for which in (R.GOAL_CENTRE, R.GOAL_ENTRY):
        goals = dev.goals(which)
        assert goals.dtype == np.int32 and len(goals) >= 1
        summary = nav.solve(cost, np_params, goals)
        want = N.solve(N.geometry(res, org[0], org[1], w, h), cost, N.params(*np_params), goals)
        assert summary == want["summary"] and nav.potential().tobytes() == want["P"].tobytes()
        assert summary["goals_used"] >= 1 and summary["goals_rejected"] == 0
    # a differing geometry is refused before any launch, and nothing changes
    before = dev.labels()
    p = R.as_tuple(R.params(R.FRONTIER))
    refused = [lambda: dev.extractFromGrids(lom.OccupancyGrid(res, org, w + 1, h), rule, None, None, p),
               lambda: dev.extractFromGrids(occ, rule, lom.ClearanceGrid(res, org, w, h - 1), None, p),
               lambda: dev.extractFromGrids(occ, rule, None, lom.NavField(res, (org[0] + 1e-6, org[1]), w, h), p),
               lambda: dev.extractFromGrids(occ, O.rule(0, 1, 1), None, None, p),
               lambda: dev.extractFromGrids(occ, rule, clear, None, R.as_tuple(R.params(R.FRONTIER, rank=R.RANK_POTENTIAL)))]
    for call in refused:
        with pytest.raises(lom.LomError) as e:
            call()
        assert e.value.code == lom.capi.ERR_ARG
    assert dev.labels().tobytes() == before.tobytes()


def test_device_form_and_a_callers_event(lom):
    import torch

    w, h = 129, 65
    rng = np.random.default_rng(12)
    plane, cost, pot = RS.frontier_plane(w, h), S.random_plane(rng, w, h, obstacles=0.1), potential_plane(rng, w, h)
    p = R.params(R.FRONTIER, max_cost=80, rank=R.RANK_POTENTIAL)
    ref = reference("device_form", plane, p, cost, pot)
    dev = lom.RegionGrid(RES, ORIGIN, w, h)
    t, c, u = (torch.from_numpy(a).to("cuda:0") for a in (plane, cost, pot.view(np.int32)))
    torch.cuda.synchronize()
    assert dev.extract(t.data_ptr(), R.as_tuple(p), c.data_ptr(), u.data_ptr(), device=True) == ref["summary"]
    assert dev.labels().tobytes() == ref["labels"].tobytes() and dev.list().tobytes() == ref["list"].tobytes()
    # planes produced on another stream: the extract waits for the caller's event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.ones(1 << 24, device="cuda:0")
        for _ in range(10):                                          # work in front of the plane
            big = big * 1.0001 + 1.0
        t2 = torch.from_numpy(plane).to("cuda:0", non_blocking=True) + 0
        ev = torch.cuda.Event()
        ev.record(s)
    late = lom.RegionGrid(RES, ORIGIN, w, h)
    assert late.extract(t2.data_ptr(), R.as_tuple(p), c.data_ptr(), u.data_ptr(), device=True,
                        hip_event=C.c_void_p(ev.cuda_event)) == ref["summary"]
    assert late.labels().tobytes() == ref["labels"].tobytes()
    d_out = C.c_void_p()
    assert lom.capi.lib().lom_regions_labels_device(late.handle, C.byref(d_out)) == 0 and d_out.value
    torch.cuda.synchronize()


# ---- mirrors -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom):
    """lom::RegionGrid of the C++ mirror compiles with plain g++ and leaves the bytes the Python package leaves."""
    exe = cpp_program.build_with_library(tmp_path, "test_regions_mirror.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    lines = stdout.rstrip("\n").split("\n")
    got_summary = [int(v) for v in lines[-3].split()]
    got_labels = np.array([int(v) for v in lines[-2].split()], np.uint64).astype(np.uint32)
    got_list = np.array([int(v) for v in lines[-1].split()], np.uint64).reshape(-1, 15)
    # the same grid and planes here (tests/cpp/test_regions_mirror.cpp)
    w, h = 45, 37
    i = np.arange(w * h)
    plane = np.where(i % 7 == 3, 100, np.where((i % 5 == 0) | (i % 11 == 2), -1, 0)).astype(np.int8).reshape(h, w)
    pot = np.where(i % 13 == 0, N.UNREACHED, (i * 37) % 1000).astype(np.uint32).reshape(h, w)
    p = R.params(R.FRONTIER, 0, 0, 99, 2, R.RANK_POTENTIAL, R.CONNECT_4)
    dev = lom.RegionGrid(RES, ORIGIN, w, h)
    summary = dev.extract(plane, R.as_tuple(p), None, pot)
    lst = dev.list()
    assert got_summary == [summary[k] for k in R.SUMMARY_KEYS]
    assert got_labels.tobytes() == dev.labels().tobytes()
    assert got_list.tolist() == [[int(v) for v in r] for r in lst]
    ref = R.extract(plane, p, None, pot)
    assert summary == ref["summary"] and dev.labels().tobytes() == ref["labels"].tobytes() and lst.tobytes() == ref["list"].tobytes()
    assert summary["regions_listed"] >= 3
