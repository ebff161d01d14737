"""The three forms in which a cost plane reaches lom_navfield, lom_navset and lom_posefield -- a host pointer, a device pointer
with an optional event, a lom_clearance -- over all 18 entry points, through capi.lib(): every single refusal
with its code and the exact bytes of last_error, and for each adjacent pair in the order of the refusals one call to which
both apply, which gets the earlier one's code and text.  The order: a NULL handle (no text), the family's argument refusals
in their order, LOM_ERR_STATE for a re-solve without a solve, the producer's geometry, the producer's device; for the
re-solves the empty-window shortcut behind all of them; for the shift the re-solve's refusals, then LOM_ERR_RANGE of the
geometry rule.  A refused call zeroes the summary and changes nothing on any handle.  Then one successful call of each
form per operation on the same handles, the device form behind a recorded event: the three forms leave the same bytes.  The
refusal of a clearance grid on another device needs a second device and is a test of its own, skipped without one.  A
40 x 33 grid: two tile columns, the second one cut, for both tile shapes."""
import ctypes as C

import numpy as np
import pytest

from tests import posefield_scenes as S

pytestmark = pytest.mark.gpu

W, H, RES, ORG = 40, 33, 0.5, (-4.0, -4.0)
CP = (1.0, 0.3, 1.5, 0)                                 # clearance: inflation and inscribed radius, decay, flags
NP, BAD_NP = (50, 3, 400, 98, 1), (0, 3, 400, 98, 1)    # navigation field parameters; neutral 0 is refused
PP, BAD_PP = (NP, 20, 1, 200, 3), (BAD_NP, 20, 1, 200, 3)
FOOT = np.ascontiguousarray(S.RECT_5x3, np.int32)
GOALS = np.array([[6, 6], [30, 24], [38, 31]], np.int32)
OFFSETS = np.array([0, 2, 3], np.uint32)                # a set of two fields
POSE_GOALS = np.array([[6, 6, -1], [30, 24, 2], [38, 31, 6]], np.int32)
MAX_FIELDS = 2
SHIFT = (3, -2)
I32_MAX = 2 ** 31 - 1
EMPTY = (0, 0, 0, 0)
FORMS = ("host", "device", "clearance")
SUFFIX = dict(host="", device="_device", clearance="_from_clearance")
ENTRIES = [(fam, op, form) for fam, ops in (("navfield", ("solve", "resolve", "shift_resolve")), ("posefield", ("solve", "resolve")),
                                            ("navset", ("solve",))) for op in ops for form in FORMS]
assert len(ENTRIES) == 18

NAV_RULE = ("neutral >= 1, 0 <= max_passable <= 98, neutral + 98 * factor <= 2^24 - 1, known flags, "
            "unknown_cost in 1 .. 2^24 - 1 under LOM_NAV_UNKNOWN_PASSABLE")
DIFFERS = "{}: the clearance grid's resolution, origin, width or height differs"
TEXT = dict(
    navfield=dict(plane="navigation field solve: a cost plane", params="navigation field parameters: " + NAV_RULE,
                  kind="navigation field: goals are LOM_NAV_CELLS or LOM_NAV_METRES",
                  goals="navigation field solve: goals, at most 2^24 of them", replane="navigation field re-solve: a cost plane",
                  state="navigation field re-solve: no solve has completed since create or clear",
                  differs=DIFFERS.format("navigation field"), shifted=DIFFERS.format("navigation field") + " from the shifted geometry",
                  elsewhere="navigation field: the clearance grid lives on another device",
                  range="navigation field: shift: the origin moved by (dx, dy) cells is not finite"),
    posefield=dict(plane="pose field solve: a cost plane",
                   params="pose field parameters: nav by the navigation field's rule, turn_cost, spin_cost, reverse_cost <= 2^24 - 1, "
                          "spin_cost >= 1 under LOM_POSE_SPIN, known flags",
                   footprint="pose field solve: a footprint of 1 .. 1024 samples with |fx|, |fy| <= 16384",
                   goals="pose field solve: goals, at most 2^24 of them", replane="pose field re-solve: a cost plane",
                   state="pose field re-solve: no solve has completed since create, clear or shift",
                   differs=DIFFERS.format("pose field"), elsewhere="pose field: the clearance grid lives on another device"),
    navset=dict(plane="navigation field set solve: a cost plane", params="navigation field set parameters: " + NAV_RULE,
                kind="navigation field set: goals are LOM_NAV_CELLS or LOM_NAV_METRES",
                too_many="navigation field set solve: n_fields is 0 .. max_fields",
                no_offsets="navigation field set solve: goal_offsets, n_fields + 1 of them",
                start="navigation field set solve: goal_offsets start at 0", fall="navigation field set solve: goal_offsets never fall",
                count="navigation field set solve: at most 2^24 goals", goals="navigation field set solve: goals",
                differs=DIFFERS.format("navigation field set"), elsewhere="navigation field set: the clearance grid lives on another device"))
# the argument refusals of a solve behind the plane's, in their order
SOLVE_ARGS = dict(navfield=("params", "kind", "goals"), posefield=("params", "footprint", "goals"),
                  navset=("params", "kind", "too_many", "no_offsets", "start", "fall", "count", "goals"))
BAD_OFFSETS = dict(start=np.array([1, 2, 3], np.uint32), fall=np.array([0, 2, 1], np.uint32), count=np.array([0, 2, 2 ** 24 + 1], np.uint32))


class Source:
    """the cost plane a clearance grid holds, in its three forms; the copy in HBM is made on a stream of its own, with an
    event recorded behind it"""

    def __init__(self, clear):
        import torch

        self.clear, self.host = clear, np.ascontiguousarray(clear.cost()[0])
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            self.device = torch.from_numpy(self.host).to("cuda:0", non_blocking=True) + 0
            self.event = torch.cuda.Event()
            self.event.record(stream)
        torch.cuda.synchronize()

    def head(self, form, event=False):
        """what stands for the plane in the call; the device form with a NULL event, or with the recorded one"""
        ev = C.c_void_p(self.event.cuda_event) if event else None
        return dict(host=(self.host.ctypes.data,), device=(self.device.data_ptr(), ev), clearance=(self.clear.handle,))[form]


def null_head(form):
    return (None, None) if form == "device" else (None,)


def call(lom, fam, op, form, handle, head, bad=(), window=None, shift=(0, 0), n_fields=2):
    """one of the 18 entry points over a poisoned summary: (return code, summary)"""
    capi = lom.capi
    sm = (capi.NavFieldSummary * 3)() if fam == "navset" else capi.PoseFieldSummary() if fam == "posefield" else capi.NavFieldSummary()
    C.memset(C.byref(sm), 0xAB, C.sizeof(sm))
    win = None if window is None else C.byref(capi.ClearanceWindow(*window))
    if op == "solve" and fam == "posefield":
        p = lom.posefieldParams(BAD_PP if "params" in bad else PP)
        tail = (C.byref(p), None if "footprint" in bad else FOOT.ctypes.data, len(FOOT), None if "goals" in bad else POSE_GOALS.ctypes.data,
                len(POSE_GOALS), C.byref(sm))
    elif op == "solve":
        p = lom.navfieldParams(BAD_NP if "params" in bad else NP)
        tail = (C.byref(p), 7 if "kind" in bad else capi.NAV_CELLS, None if "goals" in bad else GOALS.ctypes.data)
        if fam == "navfield":
            tail += (len(GOALS), C.byref(sm))
        else:
            offsets = next((BAD_OFFSETS[b] for b in bad if b in BAD_OFFSETS), OFFSETS)
            tail += (None if "no_offsets" in bad else offsets.ctypes.data, MAX_FIELDS + 1 if "too_many" in bad else n_fields, sm)
    else:
        tail = (win, C.byref(sm))
    pre = tuple(shift) if op == "shift_resolve" else ()
    return getattr(capi.lib(), f"lom_{fam}_{op}{SUFFIX[form]}")(handle, *pre, *head, *tail), sm


def geometry_bits(lom, fam, dev):
    g = lom.capi.OccupancyGeometry()
    assert getattr(lom.capi.lib(), f"lom_{fam}_get_geometry")(dev.handle, C.byref(g)) == 0
    return bytes(g)


def fields_of(fam, dev):
    """what a solve leaves on the device, as bytes"""
    if fam == "navfield":
        return [dev.potential().tobytes()]
    if fam == "navset":
        return [dev.potential(i).tobytes() for i in range(dev.fieldCount())]
    return [dev.potential().tobytes(), dev.layers().tobytes()] + [a.tobytes() for a in dev.floor()]


def state_of(lom, fam, dev):
    """everything a refused call must leave as it was"""
    stats = [dev.stats()] + ([dev.resolveStats()] if fam != "navset" else []) + ([dev.shiftStats()] if fam == "navfield" else [])
    return fields_of(fam, dev), stats, geometry_bits(lom, fam, dev)


class World:
    """one clearance grid and one solved and one fresh handle per family; a clearance grid of another width; a navigation
    field whose origin the geometry rule cannot move, solved and fresh"""

    def __init__(self, lom):
        rng = np.random.default_rng(5)
        self.lom = lom
        self.occ = [np.where(rng.random((H, W)) < 0.06, 100, 0).astype(np.int8) for _ in range(3)]
        for occ in self.occ:  # free ground about the first two goals, wide enough for the footprint, the inflation and SHIFT
            occ[:18, :18] = occ[14:, 18:] = 0
        self.clear = lom.ClearanceGrid(RES, ORG, W, H)
        self.clear.update(self.occ[0], None, CP)
        self.a = Source(self.clear)
        self.other = lom.ClearanceGrid(RES, ORG, W + 1, H)
        new = dict(navfield=lambda **k: lom.NavField(RES, ORG, W, H, **k), posefield=lambda **k: lom.PoseField(RES, ORG, W, H, **k),
                   navset=lambda **k: lom.NavFieldSet(RES, ORG, W, H, MAX_FIELDS, **k))
        self.solved = {fam: make() for fam, make in new.items()}
        self.fresh = {fam: make() for fam, make in new.items()}
        self.stuck = dict(solved=lom.NavField(1e30, (3e38, 0.0), W, H), fresh=lom.NavField(1e30, (3e38, 0.0), W, H))
        self.first = {fam: self.solve(fam, "host") for fam in new}
        rc, _ = call(lom, "navfield", "solve", "host", self.stuck["solved"].handle, self.a.head("host"))
        assert rc == 0

    def solve(self, fam, form, dev=None, event=False):
        """the plane of `a` into the solved handle of the family: the summary bytes"""
        rc, sm = call(self.lom, fam, "solve", form, (dev or self.solved[fam]).handle, self.a.head(form, event))
        assert rc == 0, (fam, form, rc)
        return bytes(sm)


@pytest.fixture(scope="module")
def world(lom):
    return World(lom)


def rows_of(world, fam, op, form):
    """(what, handle, head, keywords of call, code, text) for every refusal of the entry and for the adjacent pairs"""
    capi, t = world.lom.capi, TEXT[fam]
    ok, null, other = world.a.head(form), null_head(form), (world.other.handle,)
    solved, fresh = world.solved[fam], world.fresh[fam]
    rows = []
    if op == "solve":
        order = SOLVE_ARGS[fam]
        rows.append(("no plane", solved, null, {}, capi.ERR_ARG, t["plane"]))
        rows.append(("no plane, bad parameters", solved, null, dict(bad=("params",)), capi.ERR_ARG, t["plane"]))
        for k, b in enumerate(order):
            rows.append((b, solved, ok, dict(bad=(b,)), capi.ERR_ARG, t[b]))
            if k + 1 < len(order):
                rows.append((b + ", " + order[k + 1], solved, ok, dict(bad=(b, order[k + 1])), capi.ERR_ARG, t[b]))
        if form == "clearance":
            rows.append(("another width", solved, other, {}, capi.ERR_ARG, t["differs"]))
            rows.append(("no goals, another width", solved, other, dict(bad=("goals",)), capi.ERR_ARG, t["goals"]))
            if fam == "navset":
                rows.append(("another width, no fields", solved, other, dict(n_fields=0), capi.ERR_ARG, t["differs"]))
        return rows
    shifts = ((0, 0), SHIFT) if op == "shift_resolve" else ((0, 0),)
    for s in shifts:
        k = dict(shift=s)
        rows.append(("no plane", solved, null, k, capi.ERR_ARG, t["replane"]))
        rows.append(("no plane, no solve", fresh, null, k, capi.ERR_ARG, t["replane"]))
        rows.append(("no solve", fresh, ok, k, capi.ERR_STATE, t["state"]))
        if form == "clearance":
            differs = t["shifted"] if s != (0, 0) else t["differs"]
            rows.append(("another width", solved, other, k, capi.ERR_ARG, differs))
            rows.append(("no solve, another width", fresh, other, k, capi.ERR_STATE, t["state"]))
            rows.append(("another width, an empty window", solved, other, dict(k, window=EMPTY), capi.ERR_ARG, differs))
            if s != (0, 0):  # the clearance grid has not been shifted
                rows.append(("not shifted", solved, ok, k, capi.ERR_ARG, differs))
    if op == "shift_resolve":
        k = dict(shift=(I32_MAX, 0))
        rows.append(("an origin that is not finite", world.stuck["solved"], ok, k, capi.ERR_RANGE, t["range"]))
        rows.append(("no solve, an origin that is not finite", world.stuck["fresh"], ok, k, capi.ERR_STATE, t["state"]))
        if form == "clearance":
            rows.append(("an origin that is not finite, another width", world.stuck["solved"], other, k, capi.ERR_RANGE, t["range"]))
    return rows


@pytest.mark.parametrize("fam,op,form", ENTRIES, ids=["{}_{}{}".format(f, o, SUFFIX[m]) for f, o, m in ENTRIES])
def test_every_refusal_and_each_adjacent_pair(lom, world, fam, op, form):
    L = lom.capi.lib()
    last_error = getattr(L, f"lom_{fam}_last_error")
    # a NULL handle: no text to read, and the summary is zeroed where its length needs no handle
    rc, sm = call(lom, fam, op, form, None, world.a.head(form), shift=SHIFT)
    assert rc == lom.capi.ERR_ARG and (fam == "navset" or bytes(sm) == bytes(C.sizeof(sm)))
    rows = rows_of(world, fam, op, form)
    handles = {id(dev): dev for _, dev, *_ in rows}
    producers = [p.cost()[0].tobytes() for p in (world.clear, world.other)]
    before = {k: state_of(lom, fam, dev) for k, dev in handles.items()}
    for what, dev, head, keywords, code, text in rows:
        rc, sm = call(lom, fam, op, form, dev.handle, head, **keywords)
        assert rc == code, (what, rc)
        assert last_error(dev.handle) == text.encode(), (what, last_error(dev.handle))
        zeroed = C.sizeof(lom.capi.NavFieldSummary) * min(MAX_FIELDS, keywords.get("n_fields", 2)) if fam == "navset" else C.sizeof(sm)
        assert bytes(sm)[:zeroed] == bytes(zeroed), what
    for k, dev in handles.items():
        assert state_of(lom, fam, dev) == before[k]
    assert [p.cost()[0].tobytes() for p in (world.clear, world.other)] == producers


RESOLVES = [e for e in ENTRIES if e[1] != "solve"]


@pytest.mark.parametrize("fam,op,form", RESOLVES, ids=["{}_{}{}".format(f, o, SUFFIX[m]) for f, o, m in RESOLVES])
def test_an_empty_window_on_a_solved_field(lom, world, fam, op, form):
    """LOM_OK, the kept summary with no goal rejected, zeroed counters, the field's bytes as they were; a zero shift reports
    every cell kept"""
    dev = world.solved[fam]
    kept = world.solve(fam, "host")
    fields, geo = fields_of(fam, dev), geometry_bits(lom, fam, dev)
    rc, sm = call(lom, fam, op, form, dev.handle, world.a.head(form), window=EMPTY)
    assert rc == 0
    want = type(sm).from_buffer_copy(kept)
    want.goals_rejected = 0
    assert bytes(sm) == bytes(want) and sm.cells_reached > 100
    assert set(dev.resolveStats().values()) == {0}
    assert fields_of(fam, dev) == fields and geometry_bits(lom, fam, dev) == geo
    if op == "shift_resolve":
        assert dev.shiftStats() == dict(cells_kept=W * H, cells_entered=0, goals_left=0)


def test_a_zero_shift_whose_resolve_refuses_restores_the_geometry(lom, world):
    """the rule would make an origin of -0 a +0: a refusal behind it puts the -0 back"""
    dev = lom.NavField(RES, (-0.0, -4.0), W, H)
    world.solve("navfield", "host", dev)
    before = state_of(lom, "navfield", dev)
    assert np.signbit(dev.geometry()["origin_x"])
    rc, _ = call(lom, "navfield", "shift_resolve", "clearance", dev.handle, (world.other.handle,))
    assert rc == lom.capi.ERR_ARG
    assert lom.capi.lib().lom_navfield_last_error(dev.handle) == TEXT["navfield"]["differs"].encode()
    assert state_of(lom, "navfield", dev) == before and np.signbit(dev.geometry()["origin_x"])


FROM_CLEARANCE = [e for e in ENTRIES if e[2] == "clearance"]


@pytest.mark.parametrize("fam,op,form", FROM_CLEARANCE, ids=["{}_{}{}".format(f, o, SUFFIX[m]) for f, o, m in FROM_CLEARANCE])
def test_a_clearance_grid_on_another_device(lom, world, fam, op, form):
    """the producer's device comes behind the producer's geometry and, for a re-solve, before the empty-window shortcut"""
    if lom.capi.lib().lom_device_count() < 2:
        pytest.skip("needs a second device")
    far, far_other = lom.ClearanceGrid(RES, ORG, W, H, device=1), lom.ClearanceGrid(RES, ORG, W + 1, H, device=1)
    dev, t = world.solved[fam], TEXT[fam]
    world.solve(fam, "host")
    before = state_of(lom, fam, dev)
    window = dict(window=EMPTY) if op != "solve" else {}
    for head, text in (((far.handle,), t["elsewhere"]), ((far_other.handle,), t["differs"])):
        rc, sm = call(lom, fam, op, form, dev.handle, head, **window)
        assert rc == lom.capi.ERR_ARG and getattr(lom.capi.lib(), f"lom_{fam}_last_error")(dev.handle) == text.encode(), text
    assert state_of(lom, fam, dev) == before


def test_the_three_forms_leave_the_same_bytes(lom, world):
    """on the handles of the table: a solve per family, a re-solve of a changed plane, a shift with a re-solve behind a
    shifted and updated clearance grid -- each in all three forms from the same state"""
    clear = world.clear
    left = {}
    for fam, op, form in ENTRIES:
        dev = world.solved[fam]
        if op == "solve":
            left[fam, op, form] = (world.solve(fam, form, event=True), fields_of(fam, dev))
    clear.update(world.occ[1], None, CP)
    b = Source(clear)
    assert b.host.tobytes() != world.a.host.tobytes()
    for fam, op, form in ENTRIES:
        dev = world.solved[fam]
        if op == "resolve":
            world.solve(fam, "host")
            rc, sm = call(lom, fam, op, form, dev.handle, b.head(form, event=True), window=(3, 2, 35, 30))
            assert rc == 0 and dev.resolveStats()["cells_changed"] > 20
            left[fam, op, form] = (bytes(sm), fields_of(fam, dev), dev.resolveStats()["cells_changed"])
    clear.shift(*SHIFT)
    clear.update(world.occ[2], None, CP)
    c = Source(clear)
    dev = world.solved["navfield"]
    for form in FORMS:
        world.solve("navfield", "host")
        rc, sm = call(lom, "navfield", "shift_resolve", form, dev.handle, c.head(form, event=True), window=(3, 2, 35, 30), shift=SHIFT)
        assert rc == 0 and geometry_bits(lom, "navfield", dev) == geometry_bits(lom, "clearance", clear)
        st = dev.shiftStats()
        assert st["cells_kept"] == (W - 3) * (H - 2) and st["cells_entered"] == W * H - st["cells_kept"]
        left["navfield", "shift_resolve", form] = (bytes(sm), fields_of("navfield", dev), st, dev.resolveStats()["cells_changed"])
        dev.shift(-SHIFT[0], -SHIFT[1])
    # the world as the other tests found it
    clear.shift(-SHIFT[0], -SHIFT[1])
    clear.update(world.occ[0], None, CP)
    assert clear.cost()[0].tobytes() == world.a.host.tobytes()
    world.solve("navfield", "host")
    for fam, op, _ in ENTRIES:
        host, device, from_clearance = (left[fam, op, form] for form in FORMS)
        assert host == device == from_clearance, (fam, op)
        summary = (lom.capi.PoseFieldSummary if fam == "posefield" else lom.capi.NavFieldSummary).from_buffer_copy(host[0])
        assert summary.cells_reached > 100, (fam, op)
