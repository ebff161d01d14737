"""The pose field's re-solve on the device against tests/posefield_resolve_ref.py: the layers, the field, the floor with its
headings, the summary, cells_changed, states_changed, states_raised (the default form), the paths and the query -- all as
bytes, with no tolerance, for every case of tests/posefield_resolve_cases.py under both forms, inner cap 1 and the default,
all tiles on and off (and batch 1 and 8 on one shape).  Every case hands over garbage outside its window.  The references
of a case are computed once and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import posefield_ref as R
from tests import posefield_resolve_cases as T
from tests import posefield_resolve_ref as Q
from tests import posefield_scenes as S
from tests import rollout_ref as X

pytestmark = pytest.mark.gpu

RES, ORIGIN = T.RES, T.ORIGIN
FORMS = (0, 1)
# inner cap (0: the default), all tiles
SWITCHES = [(cap, every) for cap in (1, 0) for every in (0, 1)]
ZERO_STATS = dict(cells_changed=0, states_changed=0, states_raised=0, raise_launches=0, relax_launches=0, waits=0, tiles_marked=0)


def set_switches(lom, dev, form, cap, every, batch=0):
    dev.setOption(lom.capi.POSE_OPT_TEST_RESOLVE_FORM, form)
    dev.setOption(lom.capi.POSE_OPT_TEST_INNER_CAP, cap)
    dev.setOption(lom.capi.POSE_OPT_TEST_ALL_TILES, every)
    dev.setOption(lom.capi.POSE_OPT_TEST_BATCH, batch)


def check_state(dev, ref, what):
    """what a solve or a re-solve left against the reference: layers, field, floor, floor heading"""
    got = dev.layers()
    assert got.tobytes() == ref["L"].tobytes(), (what, "layers", np.argwhere(got != ref["L"])[:10])
    got = dev.potential()
    assert got.tobytes() == ref["P"].tobytes(), (what, "field", np.argwhere(got != ref["P"])[:10])
    fl, fh = dev.floor()
    assert fl.tobytes() == ref["floor"].tobytes(), (what, "floor")
    assert fh.tobytes() == ref["floor_heading"].tobytes(), (what, "floor heading")


def check_resolve(dev, ref, given, window, form, what, device_summary=None):
    """a re-solve of `given` over `window` on a field that holds the kept state, against the reference"""
    summary = dev.resolve(given, window) if device_summary is None else device_summary
    st = dev.resolveStats()
    check_state(dev, ref, what)
    assert summary == ref["summary"], (what, summary, ref["summary"])
    _, h, w = ref["P"].shape
    if Q.clip(w, h, window) is None:
        assert st == ZERO_STATS, (what, st)
        return st
    assert st["cells_changed"] == ref["cells_changed"], (what, st)
    if ref["cells_changed"] == 0:                                       # one wait for the diff, nothing behind it
        assert st == dict(ZERO_STATS, waits=1), (what, st)
        return st
    assert st["states_changed"] == ref["states_changed"], (what, st, ref["states_changed"])
    assert st["relax_launches"] >= 1 and st["waits"] >= 3 and st["tiles_marked"] <= -(-w // T.TILE[0]) * -(-h // T.TILE[1]), (what, st)
    if form == 0:
        assert st["states_raised"] == ref["states_raised"] and st["raise_launches"] >= 1, (what, st, ref["states_raised"])
    else:
        assert st["raise_launches"] == 0 and st["states_raised"] >= ref["states_raised"], (what, st)
    return st


def check_reads(dev, ref, p, rng, what, cap=40):
    """paths and the query read the new state"""
    _, h, w = ref["P"].shape
    starts = [(int(rng.integers(0, w)), int(rng.integers(0, h)), -1) for _ in range(5)]
    reached = np.argwhere(ref["P"] != R.UNREACHED)
    if len(reached):
        starts += [(int(x), int(y), int(hd)) for hd, y, x in reached[rng.choice(len(reached), min(5, len(reached)), replace=False)]]
    starts = np.array(starts + [(0, 0, -1), (w - 1, h - 1, 3), (-1, 0, 0), (w, h - 1, -1), (0, 0, 8)], np.int32)
    states, lengths = dev.paths(starts, cap)
    want_states, want_lengths = R.paths(ref, p, starts, cap)
    assert np.array_equal(lengths, want_lengths), (what, lengths, want_lengths)
    assert states.tobytes() == want_states.tobytes(), what
    xy = np.concatenate([rng.uniform(ORIGIN[0] - 1.0, ORIGIN[0] + w * RES + 1.0, (40, 1)),
                         rng.uniform(ORIGIN[1] - 1.0, ORIGIN[1] + h * RES + 1.0, (40, 1))], axis=1).astype(np.float32)
    hd = rng.integers(-2, 10, 40).astype(np.int32)
    assert np.array_equal(dev.query(xy, hd), R.query(T.geo_of(w, h), ref, xy, hd)), what


# ---- 1: shapes x cases x forms x switches --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", T.SHAPES)
def test_shapes_cases_forms_and_switches(lom, w, h):
    rng = np.random.default_rng(w + 7 * h)
    dev = lom.PoseField(RES, ORIGIN, w, h)
    batches = (1, 8, 0) if (w, h) == (33, 9) else (0,)
    cases = T.cases(w, h)
    assert len(cases) >= 20
    for c in cases:
        first, ref = T.references(c)
        given = T.given_plane(c)
        assert np.array_equal(Q.merged_plane(c["kept"], given, c["window"]), ref["plane"])
        raised = {}
        for form in FORMS:
            for cap, every in SWITCHES:
                for batch in batches:
                    set_switches(lom, dev, form, 0, 0)                   # (the solve in front is not what the case is about)
                    assert dev.solve(c["kept"], R.as_tuple(c["p"]), c["fp"], c["goals"]) == first["summary"], c["name"]
                    set_switches(lom, dev, form, cap, every, batch)
                    st = check_resolve(dev, ref, given, c["window"], form, (c["name"], form, cap, every, batch))
                    raised.setdefault(form, st["states_raised"])
                    assert st["states_raised"] == raised[form], (c["name"], form, cap, every, batch)   # of the form, not of the schedule
        check_reads(dev, ref, c["p"], rng, c["name"])
        # a second re-solve of the same plane finds nothing changed: the kept plane is the merged one
        again = dev.resolve(ref["plane"], None)
        assert again == dict(ref["summary"], goals_rejected=0), c["name"]
        assert dev.resolveStats() == dict(ZERO_STATS, waits=1), c["name"]
        check_state(dev, ref, (c["name"], "again"))


# ---- 2: a chain of re-solves on one handle -----------------------------------------------------------------------------------------
def test_a_chain_of_eight_resolves(lom):
    """random windows of random planes, one after another on one handle per form: each equals the reference's re-solve of the
    plane as merged so far -- a stale kept plane, stale layers, stale marks or a wrong launch parity would show"""
    w, h = 65, 17
    rng = np.random.default_rng(77)
    geo, p, fp = T.geo_of(w, h), T.P_BOTH, S.RECT_5x3
    kept = S.sparse(rng, w, h, 0.02)
    goals = T.goals_on(kept, p, fp)
    old = R.solve(geo, kept, p, fp, goals)
    devs = {form: lom.PoseField(RES, ORIGIN, w, h) for form in FORMS}
    for form, dev in devs.items():
        set_switches(lom, dev, form, 0, 0)
        assert dev.solve(kept, R.as_tuple(p), fp, goals) == old["summary"]
    changed = raised = 0
    for k in range(8):
        window = (int(rng.integers(-4, w)), int(rng.integers(-4, h)), int(rng.integers(1, 24)), int(rng.integers(1, 12)))
        new = S.sparse(rng, w, h, float(rng.choice([0.0, 0.02, 0.1])))
        ref = Q.resolve(geo, kept, new, window, p, fp, old)
        c = dict(w=w, h=h, new=new, window=window)
        for form, dev in devs.items():
            if k % 4 == 3:
                set_switches(lom, dev, form, 1, k % 8 == 7)
            check_resolve(dev, ref, T.given_plane(c, seed=k), window, form, (k, form))
        kept, old, changed, raised = ref["plane"], ref, changed + ref["cells_changed"], raised + ref["states_raised"]
    assert changed > 100 and raised > 100 and ref["summary"]["states_reached"] > 100
    check_reads(devs[0], ref, p, rng, "chain")


# ---- 3: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_zero_the_summary(lom):
    w, h = 65, 17
    rng = np.random.default_rng(31)
    p, fp = T.P_BOTH, S.RECT_5x3
    plane, other = S.sparse(rng, w, h, 0.02), S.sparse(rng, w, h, 0.05)
    goals = T.goals_on(plane, p, fp)
    dev = lom.PoseField(RES, ORIGIN, w, h)
    L, sm = lom.capi.lib(), lom.capi.PoseFieldSummary()
    zero = dict.fromkeys(R.SUMMARY_KEYS, 0)

    def refused(code, call, *args):
        sm.states_blocked = 9
        assert call(dev.handle, *args, C.byref(sm)) == code
        assert sm.asdict() == zero and L.lom_posefield_last_error(dev.handle)

    # before any solve
    refused(lom.capi.ERR_STATE, L.lom_posefield_resolve, other.ctypes.data, None)
    with pytest.raises(lom.LomError) as e:
        dev.resolve(other)
    assert e.value.code == lom.capi.ERR_STATE and (dev.potential() == R.UNREACHED).all() and dev.resolveStats() == ZERO_STATS
    first = R.solve(T.geo_of(w, h), plane, p, fp, goals)
    assert dev.solve(plane, R.as_tuple(p), fp, goals) == first["summary"]
    ref = Q.resolve(T.geo_of(w, h), plane, other, (5, 2, 30, 10), p, fp, first)
    check_resolve(dev, ref, other, (5, 2, 30, 10), 0, "before the refusals")
    stats, paths = dev.resolveStats(), dev.paths(goals, 30)
    assert stats["cells_changed"] > 100
    clear_other = lom.ClearanceGrid(RES, ORIGIN, w + 1, h)
    refused(lom.capi.ERR_ARG, L.lom_posefield_resolve, None, None)
    refused(lom.capi.ERR_ARG, L.lom_posefield_resolve_device, None, None, None)
    refused(lom.capi.ERR_ARG, L.lom_posefield_resolve_from_clearance, None, None)
    refused(lom.capi.ERR_ARG, L.lom_posefield_resolve_from_clearance, clear_other.handle, None)
    with pytest.raises(ValueError):
        dev.resolve(other[:-1])
    with pytest.raises(lom.LomError):
        dev.setOption(lom.capi.POSE_OPT_TEST_RESOLVE_FORM, 2)
    after = dev.paths(goals, 30)
    check_state(dev, ref, "after the refusals")
    assert dev.resolveStats() == stats
    assert after[0].tobytes() == paths[0].tobytes() and np.array_equal(after[1], paths[1])
    # the field still re-solves: nothing of the refused calls stuck
    ref2 = Q.resolve(T.geo_of(w, h), ref["plane"], plane, None, p, fp, ref)
    check_resolve(dev, ref2, plane, None, 0, "after the refusals")
    # after a clear and after a shift there is no solve to stand on
    dev.clear()
    refused(lom.capi.ERR_STATE, L.lom_posefield_resolve, other.ctypes.data, None)
    refused(lom.capi.ERR_STATE, L.lom_posefield_resolve_device, other.ctypes.data, None, None)
    assert (dev.potential() == R.UNREACHED).all()
    assert dev.solve(plane, R.as_tuple(p), fp, goals) == first["summary"]
    dev.shift(0, 0)
    refused(lom.capi.ERR_STATE, L.lom_posefield_resolve, other.ctypes.data, None)


# ---- 4: the three forms of the call, and the chain to the rollouts -------------------------------------------------------------------
def test_three_forms_and_the_chain_behind_a_windowed_update(lom):
    """a stream per handle: the clearance grid updates a window, one pose field re-solves from it, one from the host plane and
    one from a plane in HBM behind the caller's event; each equals the references' chain (tests/clearance_ref.py, then the
    re-solve of its cost plane).  The rollouts then read the re-solved floor as their potential."""
    import torch

    rng = np.random.default_rng(23)
    w, h = 65, 33
    cgeo, geo = K.geometry(RES, ORIGIN[0], ORIGIN[1], w, h), T.geo_of(w, h)
    p, fp = T.P_BOTH, S.RECT_5x3
    clear = lom.ClearanceGrid(RES, ORIGIN, w, h)
    a, b, c = (lom.PoseField(RES, ORIGIN, w, h) for _ in range(3))
    occ = np.where(rng.random((h, w)) < 0.01, 100, 0).astype(np.int8)
    cp = K.params(1.0, 0.3, 1.5)
    table, state = lom.clearanceCostTable(cp, RES), K.empty_state(cgeo)
    clear.update(occ, None, cp)
    want = K.update(cgeo, occ, None, cp, None, state, table)
    state = dict(d2=want["d2"], cost=want["cost"])
    goals = T.goals_on(want["cost"], p, fp, 2)
    old = R.solve(geo, want["cost"], p, fp, goals)
    assert a.solveFromClearance(clear, R.as_tuple(p), fp, goals) == old["summary"]
    assert b.solve(want["cost"], R.as_tuple(p), fp, goals) == old["summary"]
    assert c.solve(want["cost"], R.as_tuple(p), fp, goals) == old["summary"]
    pointers = (a.potentialDevice(), a.floorDevice())
    kept = want["cost"]
    for k, window in enumerate(((40, 10, 20, 16), (-3, 20, 30, 30), (30, 0, 9, 9))):
        r = Q.clip(w, h, window)
        occ = occ.copy()
        occ[r[1]:r[3], r[0]:r[2]] = np.where(rng.random((r[3] - r[1], r[2] - r[0])) < (0.1, 0.0, 0.2)[k], 100, 0)
        clear.update(occ, None, cp, window=window)
        want = K.update(cgeo, occ, None, cp, window, state, table)
        state = dict(d2=want["d2"], cost=want["cost"])
        ref = Q.resolve(geo, kept, want["cost"], window, p, fp, old)
        assert ref["cells_changed"] > 0, k
        given = T.given_plane(dict(w=w, h=h, new=want["cost"], window=window), seed=k)
        # NULL from the clearance grid on the last round: the work is sized by what changed, not by the window
        check_resolve(a, ref, None, window, 0, (k, "clearance"), device_summary=a.resolveFromClearance(clear, None if k == 2 else window))
        check_resolve(b, ref, given, window, 0, (k, "host"))
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            big = torch.ones(1 << 22, device="cuda:0")
            for _ in range(10):                                          # work in front of the plane
                big = big * 1.0001 + 1.0
            t_plane = torch.from_numpy(given).to("cuda:0", non_blocking=True) + 0
            ev = torch.cuda.Event()
            ev.record(stream)
        summary = c.resolve(t_plane.data_ptr(), window, device=True, hip_event=C.c_void_p(ev.cuda_event))
        check_resolve(c, ref, None, window, 0, (k, "device"), device_summary=summary)
        t_plane.fill_(100)                                               # the field keeps its own copy of the plane
        torch.cuda.synchronize()
        assert np.array_equal(clear.cost()[0], ref["plane"]), k
        kept, old = ref["plane"], ref
    assert (a.potentialDevice(), a.floorDevice()) == pointers           # valid across the calls
    check_reads(c, ref, p, rng, "device form")
    # the chain: ClearanceGrid.update(window) -> PoseField.resolveFromClearance -> RolloutGrid.evaluate with the floor as potential
    vis = lom.visibilityTable(X.TABLE)
    rfp = lom.rolloutFootprintRectangle(512, 512, 256, 128, False)
    free = np.argwhere(ref["floor"] != R.UNREACHED)
    pick = free[rng.choice(len(free), 40, replace=False)]
    states = np.stack([pick[:, 1] * 32768 + 16384, pick[:, 0] * 32768 + 16384, 8192 * ref["floor_heading"][tuple(pick.T)].astype(np.int64)], axis=1)
    cmd = np.stack([rng.integers(-6000, 12000, (150, 2)), rng.integers(-300, 300, (150, 2))], axis=2).astype(np.int16)
    xp = X.params(2, 30, 99, 30, min_steps=5, progress_weight=4, cost_weight=1, truncation_weight=100)
    wanted = X.evaluate_fast(ref["plane"], ref["floor"], states, cmd, rfp, vis, xp)
    assert not wanted["error"] and wanted["summary"]["admissible"] > 20
    roll = lom.RolloutGrid(RES, ORIGIN, w, h)
    d_cost = C.c_void_p()
    assert lom.capi.lib().lom_clearance_cost_device(clear.handle, C.byref(d_cost)) == 0
    got = roll.evaluate(d_cost.value, a.floorDevice()[0], states, cmd, rfp, X.as_tuple(xp), device=True)
    assert got[1] == wanted["summary"] and got[0].tobytes() == wanted["picks"].tobytes() and roll.records().tobytes() == wanted["records"].tobytes()
