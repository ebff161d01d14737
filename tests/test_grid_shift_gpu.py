"""The grid shift on the device against tests/grid_shift_ref.py: bytes are compared, with no tolerance anywhere.

The mover (lom_occupancy_shift, lom_elevation_shift): a grid is filled by one seeded scan, read back, shifted and read back
again; the second read-back equals the numpy shift of the first, the geometry the rule's bits, and classify / cost / layers
the references' answers over the shifted arrays.  Shapes are the smallest at which an alignment or edge case of the mover can
go wrong; on all but the two largest every pair of shifts is crossed, on 129 x 65 and 1030 x 515 a seeded sample of 40, every
one of them held against all of the above.  (At 1030 x 515 the numpy reference of the layers takes a fraction of a second
per pair, so the 40 pairs run as four cases of ten.)

Sequences of (shift, integrate) are held against the full model -- shift the arrays, then occupancy_ref / elevation_ref
integrate at the new geometry -- after every step; the chain occupancy + elevation -> clearance -> navigation field ->
rollouts is run, shifted as a whole and run again; and the five planning families' shifts leave what their clear leaves.
Only the public classes and capi are used."""
import functools

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import elevation_ref as E
from tests import grid_shift_ref as R
from tests import navfield_ref as N
from tests import occupancy_ref as O
from tests import rollout_ref as RO
from tests.rollout_scenes import commands_of, states_of

pytestmark = pytest.mark.gpu

I32_MAX, I32_MIN = R.I32_MAX, R.I32_MIN
RES, ORG, Z_REF = 0.25, (-37.5, 12.25), 0.5          # dyadic: a shift and its way back are exact
RAY = O.ray_params(z_lo=-1.0, z_hi=1.0, margin=0.0, min_range=0.01, max_range=400.0)
PNT = E.point_params(z_lo=-1.0, z_hi=1.0, min_range=0.01, max_range=400.0)
RULE = O.rule(min_free_scans=1, free_per_seen=1, min_seen_scans=1)
LAYER = E.layer_params(min_points=1, window=1)
COST = E.cost_params(max_slope=0.5, max_step=0.2, max_rough=0.1, max_span=0.6)
SMALL = [(1, 1), (1, 7), (7, 1), (3, 5), (63, 5), (64, 3), (65, 9), (200, 33)]
SAMPLED = [(129, 65), (1030, 515)]                   # the two largest: 40 seeded pairs each
BACK_LIMIT = 4096                                    # up to here a shift is undone by its opposite; beyond, a fresh handle


def axis_values(n):
    v = {0, I32_MAX, I32_MIN}
    for k in (1, 2, 3, 4, 5, 63, 64, 65, n - 1, n, n + 1):
        v |= {k, -k}
    return sorted(v)


def pairs_of(w, h):
    xs, ys = axis_values(w), axis_values(h)
    if (w, h) not in SAMPLED:
        return [(dx, dy) for dx in xs for dy in ys]
    rng = np.random.default_rng(w * 10007 + h)
    fixed = [(I32_MAX, 0), (I32_MIN, 2), (3, I32_MAX), (0, I32_MIN), (I32_MAX, I32_MIN), (I32_MIN, I32_MAX), (1, 1), (1, -1), (-1, 1), (-1, -1),
             (5, -3), (-63, 2), (64, -1), (-65, -5), (w - 1, h - 1), (-(w - 1), 1), (2, -(h - 1)), (w, 0), (0, -h), (0, 4), (-4, 0)]
    cross = [(dx, dy) for dx in xs for dy in ys if (dx, dy) not in fixed]
    picks = fixed + [cross[i] for i in rng.choice(len(cross), 40 - len(fixed), replace=False)]
    assert len(set(picks)) == 40
    for extreme in (I32_MAX, I32_MIN):
        assert any(dx == extreme for dx, _ in picks) and any(dy == extreme for _, dy in picks)
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):   # each sign combination, among the shifts that keep something
        assert any(dx * sx > 0 and dy * sy > 0 and abs(dx) < w and abs(dy) < h for dx, dy in picks)
    return picks


@functools.lru_cache(maxsize=None)
def fill_scan(w, h):
    """a scan in the sensor frame for a sensor at the middle of a w x h grid: a point well inside every cell, and as many
    again anywhere on the grid, so that no count of the kept part is trivially zero and the counts differ from cell to cell"""
    rng = np.random.default_rng(1000 * w + h)
    ix, iy = np.meshgrid(np.arange(w), np.arange(h))
    cx = (ix.ravel() + 0.5 + rng.uniform(-0.3, 0.3, w * h) - 0.5 * w) * RES
    cy = (iy.ravel() + 0.5 + rng.uniform(-0.3, 0.3, w * h) - 0.5 * h) * RES
    more = w * h if w * h < 100000 else 0
    x = np.concatenate([cx, rng.uniform(-0.5 * w, 0.5 * w, more) * RES])
    y = np.concatenate([cy, rng.uniform(-0.5 * h, 0.5 * h, more) * RES])
    z = rng.uniform(-0.4, 0.4, len(x))
    scan = np.column_stack([x, y, z]).astype(np.float32)
    scan.setflags(write=False)
    return scan


def middle_pose(geo):
    return np.array([geo["origin_x"] + 0.5 * geo["width"] * geo["resolution"], geo["origin_y"] + 0.5 * geo["height"] * geo["resolution"],
                     Z_REF, 1, 0, 0, 0], np.float64)


def elevation_cells(dev):
    return dict(zip(("count", "zmin", "zmax", "sum"), dev.cells()))


class Occ:
    name = "occupancy"

    def __init__(self, lom, w, h):
        self.dev = lom.OccupancyGrid(RES, ORG, w, h)

    def fill(self, scan, pose):
        self.dev.clear()
        self.dev.integrateCloud(scan, pose, RAY)

    def state(self):
        return dict(zip(("free", "seen"), self.dev.counts()))

    @staticmethod
    def shifted(state, dx, dy):
        return {k: R.shift_array(v, dx, dy, 0) for k, v in state.items()}

    @staticmethod
    def nonzero(state):
        return (state["free"] > 0) | (state["seen"] > 0)

    def check_derived(self, geo, state, cache):
        key = state["free"].tobytes() + state["seen"].tobytes()
        if key not in cache:
            cache[key] = O.classify(state["free"], state["seen"], RULE)
        cls, summary = self.dev.classify(RULE)
        assert cls.tobytes() == cache[key][0].tobytes() and summary == cache[key][1]


class Elev:
    name = "elevation"

    def __init__(self, lom, w, h):
        self.dev = lom.ElevationGrid(RES, ORG, w, h, Z_REF)

    def fill(self, scan, pose):
        self.dev.clear()
        self.dev.integrateCloud(scan, pose, PNT)

    def state(self):
        return elevation_cells(self.dev)

    @staticmethod
    def shifted(state, dx, dy):
        return R.shift_elevation_cells(state, dx, dy)

    @staticmethod
    def nonzero(state):
        return state["count"] > 0

    def check_derived(self, geo, state, cache):
        key = b"".join(state[k].tobytes() for k in ("count", "zmin", "zmax", "sum"))
        if key not in cache:
            cache[key] = (E.layers(geo, state, LAYER), E.cost(geo, state, LAYER, COST)[:2])
        layers, (cost, summary) = cache[key]
        got = self.dev.layers(LAYER)
        for k in E.LAYERS:
            assert got[k].tobytes() == layers[k].tobytes(), k
        got_cost, got_summary = self.dev.cost(LAYER, COST)
        assert got_cost.tobytes() == cost.tobytes() and got_summary == summary


def base_geometry(w, h):
    return dict(resolution=RES, origin_x=ORG[0], origin_y=ORG[1], width=w, height=h, z_ref=Z_REF)


PARTS = 4                                            # 1030 x 515: the 40 pairs in four cases of ten, a few seconds each
MOVER_CASES = [(w, h, None) for w, h in SMALL + SAMPLED[:1]] + [(SAMPLED[1][0], SAMPLED[1][1], part) for part in range(PARTS)]


@pytest.mark.parametrize("family", [Occ, Elev], ids=["occupancy", "elevation"])
@pytest.mark.parametrize("w,h,part", MOVER_CASES, ids=lambda v: str(v))
def test_mover(lom, family, w, h, part):
    """every pair: the state, the geometry, and classify / cost / layers over the shifted state"""
    geo = base_geometry(w, h)
    scan, pose, pairs = fill_scan(w, h), middle_pose(geo), pairs_of(w, h)
    if part is not None:
        pairs = pairs[part::PARTS]
    g, before, cache = None, None, {}
    n_kept_pairs = 0
    for dx, dy in pairs:
        if g is None:
            g = family(lom, w, h)
        assert R.geometry_bits(g.dev.geometry()) == R.geometry_bits(geo)
        g.fill(scan, pose)
        if before is None:                       # the same scan at the same pose on the same geometry: the same integers
            before = g.state()
            assert g.nonzero(before).mean() > 0.9
        g.dev.shift(dx, dy)
        status, want_geo = R.shift_geometry(geo, dx, dy)
        assert status == R.OK and R.geometry_bits(g.dev.geometry()) == R.geometry_bits(want_geo), (dx, dy)
        if family is Elev:
            assert g.dev.geometry()["z_ref"] == Z_REF
        got, want = g.state(), g.shifted(before, dx, dy)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, dx, dy, np.argwhere(got[k] != want[k])[:8])
        kept = R.kept_mask(w, h, dx, dy)
        if kept.any():                           # a mover that writes zeros cannot pass
            n_kept_pairs += 1
            assert g.nonzero(got)[kept].mean() >= 0.25, (dx, dy)
        assert not g.nonzero(got)[~kept].any()
        g.check_derived(want_geo, want, cache)
        if max(abs(dx), abs(dy)) <= BACK_LIMIT:
            g.dev.shift(-dx, -dy)
        else:
            g = None
    assert n_kept_pairs >= (1 if w * h == 1 else 4 if part is not None else 9)   # (of a part's ten pairs at least four keep something)


# ---- sequences -------------------------------------------------------------------------------------------------------------
def run_sequence(lom, w, h, res, org, steps=12):
    """twelve seeded steps of (shift, integrate one scan at a pose inside the new window), both families against the model
    after every step; returns every read-back"""
    rng = np.random.default_rng(31 * w + h)
    ogeo = O.geometry(np.float32(res), np.float32(org[0]), np.float32(org[1]), w, h)
    egeo = dict(ogeo, z_ref=np.float32(Z_REF))
    occ, elev = lom.OccupancyGrid(res, org, w, h), lom.ElevationGrid(res, org, w, h, Z_REF)
    free, seen, cells = np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32), E.empty_cells(egeo)
    ray = O.ray_params(z_lo=-1.0, z_hi=1.0, margin=0.0, min_range=0.2, max_range=0.6 * w * res)
    pnt = E.point_params(z_lo=-1.0, z_hi=1.0, min_range=0.2, max_range=0.6 * w * res)
    out, kept_nonzero = [], 0
    for step in range(steps):
        dx, dy = (0, 0) if step == 4 else (int(rng.integers(-9, 10)), int(rng.integers(-4, 5)))
        if step == 7:
            dx = w + 3                          # nothing is kept: a clear and the new geometry
        occ.shift(dx, dy)
        elev.shift(dx, dy)
        status, ogeo = R.shift_geometry(ogeo, dx, dy)
        assert status == R.OK
        egeo = R.shift_geometry(egeo, dx, dy)[1]
        free, seen, cells = R.shift_array(free, dx, dy, 0), R.shift_array(seen, dx, dy, 0), R.shift_elevation_cells(cells, dx, dy)
        kept_nonzero += int(((free > 0) | (seen > 0)).sum())
        assert R.geometry_bits(occ.geometry()) == R.geometry_bits(ogeo) and R.geometry_bits(elev.geometry()) == R.geometry_bits(egeo)
        ext_x, ext_y = w * float(np.float32(res)), h * float(np.float32(res))
        pose = np.array([float(ogeo["origin_x"]) + rng.uniform(0.2, 0.8) * ext_x, float(ogeo["origin_y"]) + rng.uniform(0.2, 0.8) * ext_y,
                         Z_REF + 0.1, np.cos(0.3 * step), 0, 0, np.sin(0.3 * step)], np.float64)
        n = 300
        scan = np.column_stack([rng.uniform(-0.6, 0.6, n) * ext_x, rng.uniform(-0.6, 0.6, n) * ext_x, rng.uniform(-0.5, 0.5, n)]).astype(np.float32)
        oref = O.integrate(ogeo, [scan], [0], pose[None], ray, free, seen)
        eref = E.integrate(egeo, [scan], [0], pose[None], pnt, cells)
        assert not oref["error"] and not eref["error"]
        assert occ.integrateCloud(scan, pose, ray) == oref["stats"] and elev.integrateCloud(scan, pose, pnt) == eref["stats"], step
        free, seen, cells = oref["free"], oref["seen"], eref["cells"]
        got_free, got_seen = occ.counts()
        assert got_free.tobytes() == free.tobytes() and got_seen.tobytes() == seen.tobytes(), step
        got_cells = elevation_cells(elev)
        for k in cells:
            assert got_cells[k].tobytes() == cells[k].tobytes(), (step, k)
        out += [got_free, got_seen] + [got_cells[k] for k in sorted(got_cells)]
    assert kept_nonzero > steps * w * h // 8     # content was carried across the shifts
    return b"".join(a.tobytes() for a in out)


@pytest.mark.parametrize("w,h,res,org", [(65, 9, 0.25, (-3.5, 8.0)), (200, 33, 0.1, (-12.3, 4.7))], ids=["65x9", "200x33"])
def test_sequences_against_the_model_twice(lom, w, h, res, org):
    assert run_sequence(lom, w, h, res, org) == run_sequence(lom, w, h, res, org)


@pytest.mark.parametrize("family", [Occ, Elev], ids=["occupancy", "elevation"])
def test_out_and_back(lom, family):
    w, h = 65, 9
    geo = base_geometry(w, h)
    g = family(lom, w, h)
    g.fill(fill_scan(w, h), middle_pose(geo))
    before = g.state()
    g.dev.shift(5, -3)
    g.dev.shift(-5, 3)
    assert R.geometry_bits(g.dev.geometry()) == R.geometry_bits(geo)             # dyadic: the bits return
    ix, iy = np.meshgrid(np.arange(w), np.arange(h))
    never_left = (ix - 5 >= 0) & (iy + 3 < h)
    assert never_left.any() and g.nonzero(before)[~never_left].any()
    got, cleared = g.state(), g.shifted(before, w, h)                           # (a shift that keeps nothing: the cleared values)
    for k in before:
        assert np.array_equal(got[k][never_left], before[k][never_left]), k      # the cells that never left
        assert np.array_equal(got[k][~never_left], cleared[k][~never_left]), k   # the cells that left and came back
        assert got[k].tobytes() == g.shifted(g.shifted(before, 5, -3), -5, 3)[k].tobytes()


# ---- the chain ---------------------------------------------------------------------------------------------------------------
CW, CH = 129, 65
C_ORG = (-16.0, -8.0)
C_RAY = O.ray_params(z_lo=-1.0, z_hi=1.0, margin=0.25, min_range=0.5, max_range=7.0)
C_PNT = E.point_params(z_lo=-1.0, z_hi=1.0, min_range=0.5, max_range=7.0)
C_LAYER = E.layer_params(1, 2)
C_COST = E.cost_params(max_slope=10.0, max_step=3.0, max_rough=3.0, max_span=5.0)
C_CP = K.params(0.6, 0.25, 2.0)
C_NP = (50, 3, 400, 98, 1)
C_GOALS = np.array([[x, y] for y in range(4, CH, 12) for x in range(5, CW, 17)], np.int32)
C_RP = RO.params(2, 40, 99, 30, min_steps=10, progress_weight=4, cost_weight=1, truncation_weight=100)
C_POSES = np.array([[-9.0, -2.0, 0.1, 1, 0, 0, 0], [-1.0, 1.5, 0.0, 0.9, 0, 0, 0.3], [6.0, -1.0, -0.1, 0.7, 0.02, -0.03, -0.6],
                    [11.0, 3.0, 0.0, 1, 0, 0, 0]], np.float64)
DIFFERS = "clearance: the {}'s resolution, origin, width or height differs"


def chain_scans():
    rng = np.random.default_rng(909)
    return [np.column_stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-1.2, 1.2, n)]).astype(np.float32)
            for n in (600, 601, 650, 700)]


def run_chain(lom, c, geo, table, tag):
    """the three calls, and every stage against its reference over the stage before's read-back (the handles are fresh or
    just shifted: the clearance grid's state is what its clear leaves)"""
    got_clear = c["clear"].updateFromGrids(c["occ"], RULE, c["elev"], C_LAYER, C_COST, C_CP)
    got_nav = c["nav"].solveFromClearance(c["clear"], C_NP, C_GOALS)
    occ, elev = c["occ"].classify(RULE)[0], c["elev"].cost(C_LAYER, C_COST)[0]
    cost, d2, pot = c["clear"].cost()[0], c["clear"].distanceSq(), c["nav"].potential()
    ref = K.update(geo, occ, elev, C_CP, None, K.empty_state(geo), table)
    assert not ref["error"] and got_clear == ref["summary"], (tag, got_clear, ref["summary"])
    assert np.array_equal(d2, ref["d2"]) and np.array_equal(cost, ref["cost"]), tag
    ref = N.solve(geo, cost, N.params(*C_NP), C_GOALS)
    assert got_nav == ref["summary"] and pot.tobytes() == ref["P"].tobytes(), (tag, got_nav, ref["summary"])
    rng = np.random.default_rng(4)
    fp = lom.rolloutFootprintRectangle(300, 200, 150, 100, True)
    states, cmd = states_of(cost, rng, 6), commands_of(rng, 50, 2)
    want = RO.evaluate_fast(cost, pot, states, cmd, fp, lom.visibilityTable(RO.TABLE), C_RP)
    picks, summary = c["roll"].evaluateFromGrids(c["clear"], c["nav"], states, cmd, fp, RO.as_tuple(C_RP))
    assert not want["error"] and summary == want["summary"] and picks.tobytes() == want["picks"].tobytes(), tag
    assert c["roll"].records().tobytes() == want["records"].tobytes(), tag
    assert got_nav["cells_reached"] > 500 and got_clear["cells_lethal"] > 50 and summary["admissible"] > 0, (tag, got_nav, got_clear, summary)
    return dict(occ=occ, elev=elev, cost=cost, pot=pot)


def test_the_chain_follows(lom):
    geo = K.geometry(RES, C_ORG[0], C_ORG[1], CW, CH)
    c = dict(occ=lom.OccupancyGrid(RES, C_ORG, CW, CH), elev=lom.ElevationGrid(RES, C_ORG, CW, CH, Z_REF),
             clear=lom.ClearanceGrid(RES, C_ORG, CW, CH), nav=lom.NavField(RES, C_ORG, CW, CH), roll=lom.RolloutGrid(RES, C_ORG, CW, CH))
    unshifted = lom.ClearanceGrid(RES, C_ORG, CW, CH)
    table = lom.clearanceCostTable(C_CP, RES)
    for scan, pose in zip(chain_scans(), C_POSES):
        c["occ"].integrateCloud(scan, pose, C_RAY)
        c["elev"].integrateCloud(scan, pose, C_PNT)
    first = run_chain(lom, c, geo, table, "before")
    for h in c.values():
        h.shift(7, -4)
    status, moved = R.shift_geometry(geo, 7, -4)
    assert status == R.OK
    for name, h in c.items():
        assert R.geometry_bits(h.geometry()) == R.geometry_bits(moved), name
    second = run_chain(lom, c, moved, table, "after")
    # the producers' planes are the first round's, moved: what entered is unknown
    assert second["occ"].tobytes() == R.shift_array(first["occ"], 7, -4, O.UNKNOWN).tobytes()
    # a consumer that was not shifted meets the shifted producers with the usual refusal
    for occupancy, elevation, who in ((c["occ"], None, "occupancy grid"), (None, c["elev"], "elevation grid")):
        with pytest.raises(lom.LomError) as e:
            unshifted.updateFromGrids(occupancy, RULE, elevation, C_LAYER, C_COST, C_CP)
        assert e.value.code == lom.capi.ERR_ARG and str(e.value).endswith(": " + DIFFERS.format(who)), str(e.value)


# ---- the five planning families --------------------------------------------------------------------------------------------------
def snapshot(lom, handles):
    """every read-back of the five handles' state, or the error it is refused with (the launches and waits of the last call,
    lom_*_stats, are an account of that call and no state: no clear touches them)"""
    calls = dict(d2=lambda: handles["clear"].distanceSq(), cost=lambda: handles["clear"].cost(), potential=lambda: handles["nav"].potential(),
                 labels=lambda: handles["reg"].labels(), reg_list=lambda: handles["reg"].list(), reg_goals=lambda: handles["reg"].goals(),
                 vis_records=lambda: handles["vis"].records(),
                 roll_records=lambda: handles["roll"].records())
    out = {}
    for name, call in calls.items():
        try:
            v = call()
        except lom.LomError as e:
            v = ("refused", e.code)
        if isinstance(v, tuple) and isinstance(v[0], np.ndarray):
            v = (v[0].tobytes(), v[1])
        out[name] = v.tobytes() if isinstance(v, np.ndarray) else v
    return out


def call_stats(handles):
    """lom_*_stats of the four families that keep an account of their last call"""
    return {k: handles[k].stats() for k in ("nav", "reg", "vis", "roll")}


def five(lom, res, org, w, h):
    return dict(clear=lom.ClearanceGrid(res, org, w, h), nav=lom.NavField(res, org, w, h), reg=lom.RegionGrid(res, org, w, h),
                vis=lom.VisibilityGrid(res, org, w, h), roll=lom.RolloutGrid(res, org, w, h))


def give_state(lom, handles, planes, clearance_params):
    """an update, a solve, an extraction, a cast and an evaluation from host planes: every handle has something to lose"""
    from tests import regions_ref as G
    from tests import test_plane_core_gpu as T
    from tests import visibility_ref as V

    rng = np.random.default_rng(4)
    handles["clear"].update(planes["occ"], planes["elev"], clearance_params)
    handles["nav"].solve(planes["cost"], T.NP, T.GOALS)
    handles["reg"].extract(planes["occ"], G.as_tuple(T.RP), planes["cost"], planes["potential"])
    handles["vis"].cast(planes["occ"], T.VP, V.as_tuple(T.VISP))
    fp = lom.rolloutFootprintRectangle(300, 200, 150, 100, True)
    handles["roll"].evaluate(planes["cost"], planes["potential"], states_of(planes["cost"], rng, 6), commands_of(rng, 20, 2), fp,
                             RO.as_tuple(C_RP))


@pytest.fixture(scope="module")
def chain_planes(lom):
    """the planes of tests/test_plane_core_gpu.py's chain after its first round, 16 x 16"""
    from tests import test_plane_core_gpu as T

    return T.Chain(lom).round(0)


def test_plane_families_shift_to_what_clear_leaves(lom, chain_planes):
    from tests import test_plane_core_gpu as T

    handles = five(lom, T.RES, T.ORG, T.W, T.H)
    give_state(lom, handles, chain_planes, T.CP)
    with_state = snapshot(lom, handles)
    for dx, dy in ((3, -2), (0, 0), (I32_MIN, 40)):
        if (dx, dy) != (3, -2):
            give_state(lom, handles, chain_planes, T.CP)
            assert snapshot(lom, handles) == with_state
        before = {k: h.geometry() for k, h in handles.items()}
        accounts = call_stats(handles)
        assert all(a["launches"] > 0 for a in accounts.values())
        for h in handles.values():
            h.shift(dx, dy)
        assert call_stats(handles) == accounts, (dx, dy)      # as after the family's own clear: the last call's account stays
        fresh = {}
        for k, h in handles.items():
            status, want = R.shift_geometry(before[k], dx, dy)
            assert status == R.OK and R.geometry_bits(h.geometry()) == R.geometry_bits(want), (k, dx, dy)
            fresh[k] = type(h)(T.RES, (float(want["origin_x"]), float(want["origin_y"])), T.W, T.H)
            assert R.geometry_bits(fresh[k].geometry()) == R.geometry_bits(want)
            fresh[k].clear()
        after = snapshot(lom, handles)
        assert after == snapshot(lom, fresh), (dx, dy)
        assert all(after[k] != with_state[k] for k in ("d2", "cost", "potential", "labels", "vis_records", "roll_records")), (dx, dy)
    # the premise of the above: a family's own clear leaves the account of its last call as it is
    give_state(lom, handles, chain_planes, T.CP)
    accounts = call_stats(handles)
    for h in handles.values():
        h.clear()
    assert call_stats(handles) == accounts


def test_a_refused_shift_changes_nothing(lom, chain_planes):
    """the overflow case: an origin of 3e38 with a resolution of 1e30 moved by 10^9 cells is not finite"""
    from tests import test_plane_core_gpu as T

    res, org = 1e30, (3e38, -4e30)
    handles = five(lom, res, org, T.W, T.H)
    give_state(lom, handles, chain_planes, K.params(1.2e30, 0.5e30, 2e-30))
    # the two grids that hold state: a sensor at x = 3e38 exactly sees points at the same x (the column ix = 0), up and down
    # the rows
    occ, elev = lom.OccupancyGrid(res, org, 8, 8), lom.ElevationGrid(res, org, 8, 8, Z_REF)
    scan = np.array([[0.0, (k - 3.6) * 1e30, 0.3] for k in range(8) if k != 4], np.float32)
    pose = np.array([3e38, 0.4e30, Z_REF, 1, 0, 0, 0], np.float64)
    occ.integrateCloud(scan, pose, O.ray_params(z_lo=-1.0, z_hi=1.0, margin=0.0, min_range=1e29, max_range=8e30))
    elev.integrateCloud(scan, pose, E.point_params(z_lo=-1.0, z_hi=1.0, min_range=1e29, max_range=8e30))
    grids = dict(occ=occ, elev=elev)
    read = lambda: (b"".join(a.tobytes() for a in occ.counts()), b"".join(a.tobytes() for a in elev.cells()))  # noqa: E731
    counts_before, planes_before = read(), snapshot(lom, handles)
    assert np.count_nonzero(occ.counts()[1]) >= 4 and np.count_nonzero(elev.cells()[0]) >= 4
    geometry_before = {k: h.geometry() for k, h in {**handles, **grids}.items()}
    for k, h in {**handles, **grids}.items():
        for dx, dy in ((1000000000, 0), (I32_MAX, -1)):
            assert R.shift_geometry(geometry_before[k], dx, dy)[0] == R.ERR_RANGE
            with pytest.raises(lom.LomError) as e:
                h.shift(dx, dy)
            assert e.value.code == lom.capi.ERR_RANGE and "shift: the origin moved by (dx, dy) cells is not finite" in str(e.value), (k, str(e.value))
        assert h.geometry() == geometry_before[k], k
    assert read() == counts_before and snapshot(lom, handles) == planes_before
    # and they still shift where the rule allows it
    for k, h in {**handles, **grids}.items():
        h.shift(-3, 2)
        assert R.geometry_bits(h.geometry()) == R.geometry_bits(R.shift_geometry(geometry_before[k], -3, 2)[1]), k
