"""What the four planning grids share on the host (csrc/plane_handle.hpp), on the device: one OccupancyGrid and one
ElevationGrid feed a ClearanceGrid, a NavField, a RegionGrid and a VisibilityGrid, every handle on a stream of its own, and
each stage reads the plane the stage before left in HBM.  Every stage equals its reference (tests/clearance_ref.py,
navfield_ref.py, regions_ref.py, visibility_ref.py) fed with the read-back of the stage before -- also in a second round,
where every producer overwrites a plane a consumer has read; and the refusals in front of the hand-off, which name their
reason in last_error and leave every handle as it was.  Only the public classes and capi are used."""
import numpy as np
import pytest

from tests import clearance_ref as K
from tests import elevation_ref as E
from tests import navfield_ref as N
from tests import occupancy_ref as O
from tests import regions_ref as R
from tests import visibility_ref as V
from tests.test_grid_core_gpu import POSES, three_scans

pytestmark = pytest.mark.gpu

RES, ORG, W, H, Z_REF = 0.5, (-4.0, -4.0), 16, 16, 0.25  # 16 x 16 cells of 0.5 m
GEO = K.geometry(RES, ORG[0], ORG[1], W, H)
# rays of 2.5 m leave the grid's rim unknown: there is a frontier, and unknown cells for the viewpoints to see
RAY = O.ray_params(z_lo=-1.0, z_hi=1.0, margin=0.25, min_range=0.5, max_range=2.5)
PNT = E.point_params(z_lo=-1.0, z_hi=1.0, min_range=0.5, max_range=6.0)
RULE, LAYER, COSTP = O.rule(1, 1, 1), E.layer_params(1, 2), E.cost_params(max_slope=10.0, max_step=3.0, max_rough=3.0, max_span=5.0)
CP = K.params(0.6, 0.25, 2.0)                                                   # one cell of inflation
NP = (50, 3, 400, 98, 1)                                                        # unknown cells are passable, at a price
GOALS = np.array([[x, y] for y in range(1, 16, 3) for x in range(1, 16, 3)], np.int32)  # some of them on obstacles
RP = R.params(R.FRONTIER, max_cost=98, min_cells=1, rank=R.RANK_POTENTIAL)
VP = np.array([[5, 5], [9, 4], [11, 7]], np.int32)                              # 3 viewpoints, 16 beams, range 6
VISP = V.params(16, 6, 100, 0, V.KEEP_WINDOWS)
SEL = V.select_params(3, 64, 4, 1)
REFS = {}

DIFFERS = "{}: the {}'s resolution, origin, width or height differs"
ELSEWHERE = "{}: the {} lives on another device"


def once(stage, compute, *inputs):
    """the reference of a stage over these inputs, computed once"""
    key = (stage,) + tuple(np.asarray(a).tobytes() for a in inputs)
    if key not in REFS:
        REFS[key] = compute()
    return REFS[key]


class Producers:
    """the four handles a stage reads from, of one geometry on one device"""

    def __init__(self, lom, res=RES, org=ORG, w=W, h=H, device=0):
        self.occ = lom.OccupancyGrid(res, org, w, h, device=device)
        self.elev = lom.ElevationGrid(res, org, w, h, Z_REF, device=device)
        self.clear = lom.ClearanceGrid(res, org, w, h, device=device)
        self.nav = lom.NavField(res, org, w, h, device=device)


class Chain(Producers):
    """occupancy, elevation -> clearance -> navigation field -> regions -> visibility, and what the references expect"""

    def __init__(self, lom):
        super().__init__(lom)
        self.lom, self.scans = lom, three_scans()
        self.reg, self.vis = lom.RegionGrid(RES, ORG, W, H), lom.VisibilityGrid(RES, ORG, W, H)
        self.state = K.empty_state(GEO)
        self.table = lom.clearanceCostTable(CP, RES)
        K.compare_table(self.table, CP, RES)
        self.beams = lom.visibilityTable(VISP["beams"])

    def run(self):
        """the five calls; the host waits for nothing but what each call waits for itself"""
        return dict(clear=self.clear.updateFromGrids(self.occ, RULE, self.elev, LAYER, COSTP, CP),
                    nav=self.nav.solveFromClearance(self.clear, NP, GOALS),
                    reg=self.reg.extractFromGrids(self.occ, RULE, self.clear, self.nav, R.as_tuple(RP)),
                    vis=self.vis.castFromOccupancy(self.occ, RULE, VP, V.as_tuple(VISP)),
                    picks=self.vis.selectFromNavfield(self.nav, V.select_tuple(SEL)))

    def read(self):
        """every result of every handle"""
        return dict(occ=self.occ.classify(RULE)[0], elev=self.elev.cost(LAYER, COSTP)[0], cost=self.clear.cost()[0], d2=self.clear.distanceSq(),
                    potential=self.nav.potential(), labels=self.reg.labels(), list=self.reg.list(), records=self.vis.records(),
                    windows=self.vis.windows(), stats=np.array([list(x.stats().values())[:2] for x in (self.nav, self.reg, self.vis)], np.uint64))

    def round(self, k):
        """scan k into the two grids, the chain, and every stage against its reference over the stage before's read-back"""
        self.occ.integrateCloud(self.scans[k], POSES[k], RAY)
        self.elev.integrateCloud(self.scans[k], POSES[k], PNT)
        got, back = self.run(), self.read()
        occ, elev, cost, pot = back["occ"], back["elev"], back["cost"], back["potential"]
        ref = once("clear", lambda: K.update(GEO, occ, elev, CP, None, self.state, self.table), occ, elev, self.state["d2"], self.state["cost"])
        assert not ref["error"] and got["clear"] == ref["summary"], (k, got["clear"], ref["summary"])
        assert np.array_equal(back["d2"], ref["d2"]) and np.array_equal(cost, ref["cost"]), k
        self.state = dict(d2=ref["d2"], cost=ref["cost"])
        ref = once("nav", lambda: N.solve(GEO, cost, N.params(*NP), GOALS), cost)
        assert got["nav"] == ref["summary"] and pot.tobytes() == ref["P"].tobytes(), (k, got["nav"], ref["summary"])
        ref = once("reg", lambda: R.extract(occ, RP, cost, pot), occ, cost, pot)
        assert got["reg"] == ref["summary"], (k, got["reg"], ref["summary"])
        assert back["labels"].tobytes() == ref["labels"].tobytes() and back["list"].tobytes() == ref["list"].tobytes(), k
        ref = once("vis", lambda: V.cast_fast(occ, VP, self.beams, VISP), occ)
        assert got["vis"] == ref["summary"], (k, got["vis"], ref["summary"])
        assert back["records"].tobytes() == ref["records"].tobytes() and back["windows"].tobytes() == ref["windows"].tobytes(), k
        assert got["picks"].tobytes() == V.select(ref, SEL, pot[VP[:, 1], VP[:, 0]]).tobytes(), k
        # the round says something: a frontier, a route to it, viewpoints that see unknown cells and are worth a visit
        assert got["reg"]["regions_listed"] >= 3 and got["nav"]["cells_reached"] > 100 and got["nav"]["goals_rejected"] >= 1
        assert got["vis"]["valid"] == 3 and got["vis"]["unknown_total"] > 10 and len(got["picks"]) == 3
        return back


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_the_chain_on_five_streams_twice(lom):
    c = Chain(lom)
    first = c.round(0)
    second = c.round(1)  # every producer overwrites a plane a consumer read in the first round
    for k in ("occ", "elev", "cost", "potential", "labels", "list", "records"):
        assert first[k].tobytes() != second[k].tobytes(), k


def refused(lom, family, consumer, call, text):
    """`call` raises LomError(LOM_ERR_ARG) with `text`, and the consumer's last error is `text`"""
    with pytest.raises(lom.LomError) as e:
        call()
    assert e.value.code == lom.capi.ERR_ARG and str(e.value).endswith(": " + text), str(e.value)
    last = getattr(lom.capi.lib(), "lom_" + family + "_last_error")(consumer.handle)
    assert last.decode() == text


def hand_offs(c, o):
    """every consumer / producer pair, the producer taken from `o`: (family, consumer's name, consumer, producer's name, call)"""
    rp, vp, sel = R.as_tuple(RP), V.as_tuple(VISP), V.select_tuple(SEL)
    return [("clearance", "clearance", c.clear, "occupancy grid", lambda: c.clear.updateFromGrids(o.occ, RULE, c.elev, LAYER, COSTP, CP)),
            ("clearance", "clearance", c.clear, "elevation grid", lambda: c.clear.updateFromGrids(c.occ, RULE, o.elev, LAYER, COSTP, CP)),
            ("navfield", "navigation field", c.nav, "clearance grid", lambda: c.nav.solveFromClearance(o.clear, NP, GOALS)),
            ("regions", "region grid", c.reg, "occupancy grid", lambda: c.reg.extractFromGrids(o.occ, RULE, c.clear, c.nav, rp)),
            ("regions", "region grid", c.reg, "clearance grid", lambda: c.reg.extractFromGrids(c.occ, RULE, o.clear, c.nav, rp)),
            ("regions", "region grid", c.reg, "navigation field", lambda: c.reg.extractFromGrids(c.occ, RULE, c.clear, o.nav, rp)),
            ("visibility", "visibility grid", c.vis, "occupancy grid", lambda: c.vis.castFromOccupancy(o.occ, RULE, VP, vp)),
            ("visibility", "visibility grid", c.vis, "navigation field", lambda: c.vis.selectFromNavfield(o.nav, sel))]


def filled_chain(lom):
    c = Chain(lom)
    c.round(0)
    return c, c.round(1)


def test_a_refused_hand_off_names_its_reason_and_changes_nothing(lom):
    c, before = filled_chain(lom)
    # one field of the producer's geometry differs: the width, the height, the resolution, the origin
    for other in (dict(w=17), dict(h=17), dict(res=0.25), dict(org=(0.5, -4.0))):
        for family, name, consumer, producer, call in hand_offs(c, Producers(lom, **other)):
            refused(lom, family, consumer, call, DIFFERS.format(name, producer))
    # bit for bit: -0.0 is not 0.0
    nav, clear = lom.NavField(RES, (0.0, -4.0), W, H), lom.ClearanceGrid(RES, (-0.0, -4.0), W, H)
    assert np.signbit(clear.geometry()["origin_x"]) and not np.signbit(nav.geometry()["origin_x"])
    refused(lom, "navfield", nav, lambda: nav.solveFromClearance(clear, NP, GOALS), DIFFERS.format("navigation field", "clearance grid"))
    assert same(before, c.read())
    c.round(2)  # and the chain still runs


def test_a_producer_on_another_device(lom):
    if lom.capi.lib().lom_device_count() < 2:
        pytest.skip("needs a second device")
    c, before = filled_chain(lom)
    for family, name, consumer, producer, call in hand_offs(c, Producers(lom, device=1)):
        refused(lom, family, consumer, call,
                "region grid: a grid lives on another device" if family == "regions" else ELSEWHERE.format(name, producer))
    assert same(before, c.read())
