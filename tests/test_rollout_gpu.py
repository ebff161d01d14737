"""The trajectory rollouts on the GPU against tests/rollout_ref.py: picks, records (as bytes) and summary are exactly the
reference's under every setting of the three test switches, over shapes, planes, (L, Tn), footprint sizes, candidate and
state counts; first blocks at the chunk border; ties; the chain ClearanceGrid -> NavField -> RolloutGrid; refused calls."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as K
from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import regions_scenes as RS
from tests import rollout_ref as R
from tests.rollout_scenes import CELL, commands_of, footprint_of, states_of

pytestmark = pytest.mark.gpu

RES, ORIGIN = 0.25, (-3.0, 2.0)
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 31), (65, 33), (129, 65)]
# (L, Tn, F, K, M): a chunk border at, before and after a segment border; F and K around a wave and far from a multiple of
# one.  With +-200 / 256 cells of footprint the window is staged in LDS for the first four and read in HBM for the last two.
CONFIGS = [(1, 1, 300, 300, 3), (1, 63, 65, 65, 8), (1, 64, 64, 300, 1), (1, 65, 63, 65, 5), (2, 65, 2, 300, 3), (8, 128, 1, 65, 4)]
# (unknown_cost, lethal_min, min_steps is S, with a potential), rotated against the planes and the configurations
MODES = [(-1, 100, False, True), (7, 50, True, False), (7, 100, False, True), (-1, 50, False, False), (-1, 100, True, True), (7, 50, False, True)]
# serial, no LDS plane, waves
SWITCHES = [(serial, no_lds, waves) for serial in (0, 1) for no_lds in (0, 1) for waves in (1, 4)]
REFS = {}


@pytest.fixture(scope="module")
def table(lom):
    return lom.visibilityTable(R.TABLE)


def reference(key, table, plane, potential, states, cmd, fp, p):
    """the reference's evaluation of a case, once"""
    if key not in REFS:
        REFS[key] = R.evaluate_fast(plane, potential, states, cmd, fp, table, p)
    return REFS[key]


def set_switches(lom, dev, serial, no_lds, waves):
    dev.setOption(lom.capi.ROLLOUT_OPT_TEST_SERIAL, serial)
    dev.setOption(lom.capi.ROLLOUT_OPT_TEST_NO_LDS_PLANE, no_lds)
    dev.setOption(lom.capi.ROLLOUT_OPT_TEST_WAVES, waves)


def planes_of(w, h):
    rng = np.random.default_rng(1000 * w + h)
    return {"free": S.empty(w, h), "unknown": np.full((h, w), -1, np.int8), "lethal": RS.full(w, h),
            "random": S.random_plane(rng, w, h, obstacles=0.01, unknown=0.02), "serpentine": S.serpentine(w, h), "pocket": S.pocket(w, h)}


def potential_of(rng, plane):
    """a potential in the field's form: a distance-like value per cell, LOM_NAV_UNREACHED on lethal cells and a few others"""
    h, w = plane.shape
    y, x = np.mgrid[0:h, 0:w]
    pot = (250 * (np.abs(x - w // 3) + np.abs(y - h // 2)) + rng.integers(0, 50, (h, w))).astype(np.uint32)
    pot[(plane >= 100) | (rng.random((h, w)) < 0.02)] = R.UNREACHED
    return pot


def check(dev, ref, plane, potential, states, cmd, fp, p, what=None):
    """one evaluation against the reference: picks, summary, records and the launches"""
    picks, summary = dev.evaluate(plane, potential, states, cmd, fp, R.as_tuple(p))
    assert not ref["error"] and summary == ref["summary"], (what, summary, ref["summary"])
    assert picks.tobytes() == ref["picks"].tobytes(), (what, picks[:6], ref["picks"][:6])
    got = dev.records()
    assert len(got) == len(ref["records"]), (what, len(got))
    if got.tobytes() != ref["records"].tobytes():
        bad = [i for i in range(len(got)) if got[i] != ref["records"][i]][:4]
        raise AssertionError((what, [(i, got[i], ref["records"][i]) for i in bad]))
    launches = 0 if not len(states) else (3 if len(cmd) else 2)
    assert dev.stats() == dict(launches=launches, waits=1 if len(states) else 0), (what, dev.stats())


# ---- 1: shapes x planes x configurations x modes x switches ---------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_shapes_planes_and_switches(lom, table, i):
    w, h = SHAPES[i]
    rng = np.random.default_rng(w + 7 * h)
    dev = lom.RolloutGrid(RES, ORIGIN, w, h)
    assert len(dev.records()) == 0 and dev.stats() == dict(launches=0, waits=0)                 # after create
    reasons, free_poses = set(), set()
    for j, (name, plane) in enumerate(planes_of(w, h).items()):
        segments, tn, f, k, m = CONFIGS[(i + j + 3) % len(CONFIGS)]
        unknown_cost, lethal_min, strict, with_potential = MODES[(i + 2 * j + j // 3) % len(MODES)]
        steps = segments * tn
        p = R.params(segments, tn, lethal_min, unknown_cost, min_steps=steps if strict else 0, progress_weight=3, cost_weight=5,
                     truncation_weight=40)
        states, cmd, fp = states_of(plane, rng, m), commands_of(rng, k, segments), footprint_of(rng, f)
        potential = potential_of(rng, plane) if with_potential else None
        ref = reference((w, h, name), table, plane, potential, states, cmd, fp, p)
        reasons |= set(ref["records"]["reason"].tolist())
        free_poses |= set(ref["records"]["free_poses"].tolist())
        for serial, no_lds, waves in SWITCHES:
            set_switches(lom, dev, serial, no_lds, waves)
            check(dev, ref, plane, potential, states, cmd, fp, p, what=(name, segments, tn, f, k, m, serial, no_lds, waves))
    if w * h > 1000:
        assert reasons == {R.OK, R.UNKNOWN, R.COLLISION, R.EDGE, R.INVALID}
        assert 0 in free_poses and max(free_poses) == 1025 and len(free_poses) > 20
        admissible = sum(REFS[(w, h, name)]["summary"]["admissible"] for name in ("free", "random", "pocket"))
        assert admissible > 50


# ---- 2: the counts 0, 1, 3 of states and 0, 1, 65, 300 of candidates, F = 1 and 2 ------------------------------------------------
def test_state_and_candidate_counts(lom, table):
    w, h = 65, 33
    rng = np.random.default_rng(3)
    plane = S.random_plane(rng, w, h, obstacles=0.02, unknown=0.03)
    potential = potential_of(rng, plane)
    dev = lom.RolloutGrid(RES, ORIGIN, w, h)
    p = R.params(2, 40, 100, 7, min_steps=3, progress_weight=2, cost_weight=1, truncation_weight=9)
    for n, (m, k, f) in enumerate([(0, 0, 1), (0, 65, 2), (1, 0, 1), (3, 0, 2), (1, 1, 1), (3, 1, 2), (1, 65, 1), (3, 300, 2), (1, 300, 1), (3, 65, 63)]):
        states, cmd, fp = states_of(plane, rng, m), commands_of(rng, k, 2), footprint_of(rng, f)
        ref = reference(("counts", m, k, f), table, plane, potential, states, cmd, fp, p)
        assert ref["summary"]["states"] == m and ref["summary"]["candidates"] == m * k and len(ref["picks"]) == m
        if not k:
            assert (ref["picks"]["k"] == R.NONE).all() and ref["summary"]["states_without_pick"] == m
        serial, no_lds, waves = SWITCHES[n % len(SWITCHES)]
        for sw in ((serial, no_lds, waves), (1 - serial, no_lds, 5 - waves)):
            set_switches(lom, dev, *sw)
            check(dev, ref, plane, potential, states, cmd, fp, p, what=(m, k, f, sw))


# ---- 3: a first block at poses 63, 64 and 65; the floor rule on the negative side; ties -----------------------------------------
def test_first_block_at_the_chunk_border_negative_side_and_ties(lom, table):
    w, h = 129, 65
    plane = S.empty(w, h)
    plane[:, 67] = 100
    # heading 0 at full speed: a step adds 32767 units, so from the middle of cell c pose t lies in cell c + t (t < 16384);
    # the wall's cell is 67: from the cells 4, 3, 2 the first blocked pose is 63, 64, 65
    states = np.array([[c * CELL + CELL // 2, 30 * CELL + 5, 0] for c in (4, 3, 2)], np.int64)
    point = np.zeros((1, 2), np.int64)
    dev = lom.RolloutGrid(RES, ORIGIN, w, h)
    for segments, tn in ((1, 65), (2, 65), (1, 64)):
        cmd = np.zeros((3, segments, 2), np.int16)
        cmd[0, :, 0], cmd[1, :, 0], cmd[2, :, 0] = 32767, 32767, 16384             # the second repeats the first: a tie
        p = R.params(segments, tn, 100, -1, min_steps=0, progress_weight=0, cost_weight=1, truncation_weight=1)
        ref = reference(("border", segments, tn), table, plane, None, states, cmd, point, p)
        want = [min(t, segments * tn + 1) for t in (63, 64, 65)]
        assert ref["records"]["free_poses"].reshape(3, 3)[:, 0].tolist() == want
        assert ref["records"]["reason"].reshape(3, 3)[:, 0].tolist() == [R.COLLISION if t <= segments * tn else R.OK for t in want]
        assert ref["records"]["end_x"].reshape(3, 3)[:, 0].tolist() == [int(s[0]) + 32767 * (t - 1) for s, t in zip(states, want)]
        assert (ref["picks"]["k"] != 1).all()                                     # of two equal candidates the lesser index
        for sw in SWITCHES:
            set_switches(lom, dev, *sw)
            check(dev, ref, plane, None, states, cmd, point, p, what=(segments, tn, sw))
    # a footprint whose samples leave the grid on the negative side by a fraction of a cell: the cell is floor, -1, not 0
    fp = np.array([[0, 0], [-130, 0], [0, -130]], np.int64)                       # half a cell behind and to the right
    states = np.array([[CELL // 2 - 1, 10 * CELL, 0], [CELL // 2 + 1000, 10 * CELL, 0], [10 * CELL, CELL // 2 - 1, 0], [10 * CELL, CELL // 2 + 1000, 0]], np.int64)
    cmd = np.zeros((2, 1, 2), np.int16)
    cmd[1, 0] = (300, 0)
    p = R.params(1, 4, 100, -1, min_steps=0, progress_weight=0, cost_weight=1, truncation_weight=1)
    ref = reference("negative", table, plane, None, states, cmd, fp, p)
    assert ref["records"]["reason"].reshape(4, 2)[:, 0].tolist() == [R.EDGE, R.OK, R.EDGE, R.OK]
    assert ref["records"]["free_poses"].reshape(4, 2)[:, 0].tolist() == [0, 5, 0, 5]
    for sw in SWITCHES:
        set_switches(lom, dev, *sw)
        check(dev, ref, plane, None, states, cmd, fp, p, what=("negative", sw))


# ---- 4: the chain, the device form, refused calls -------------------------------------------------------------------------------
def test_from_grids_the_chain_and_refused_calls(lom, table):
    rng = np.random.default_rng(21)
    w, h = 90, 47
    geo = K.geometry(RES, ORIGIN[0], ORIGIN[1], w, h)
    occ = np.where(rng.random((h, w)) < 0.01, 100, 0).astype(np.int8)
    occ[rng.random((h, w)) < 0.02] = -1
    cp = K.params(1.0, 0.3, 1.5)
    nav_params = (50, 3, 400, 98, 1)
    goals = np.array([[w - 5, h // 2], [3, 3]], np.int32)
    clear, nav = lom.ClearanceGrid(RES, ORIGIN, w, h), lom.NavField(RES, ORIGIN, w, h)
    clear.update(occ, None, cp)
    nav.solveFromClearance(clear, nav_params, goals)
    # the references' chain gives the same planes
    cost = K.update(geo, occ, None, cp, table=lom.clearanceCostTable(cp, RES))["cost"]
    potential = N.solve(N.geometry(RES, ORIGIN[0], ORIGIN[1], w, h), cost, N.params(*nav_params), goals)["P"]
    assert np.array_equal(clear.cost()[0], cost) and np.array_equal(nav.potential(), potential)
    assert (cost == 99).any() and ((cost > 0) & (cost < 99)).any() and (potential != R.UNREACHED).sum() > 1000
    fp = lom.rolloutFootprintRectangle(300, 200, 150, 100, True)
    states, cmd = states_of(cost, rng, 6), commands_of(rng, 200, 2)
    p = R.params(2, 40, 99, 30, min_steps=10, progress_weight=4, cost_weight=1, truncation_weight=100)
    ref = reference("chain", table, cost, potential, states, cmd, fp, p)
    assert ref["summary"]["admissible"] > 100 and ref["summary"]["states_without_pick"] < 6
    dev, host = lom.RolloutGrid(RES, ORIGIN, w, h), lom.RolloutGrid(RES, ORIGIN, w, h)
    for n, sw in enumerate(SWITCHES[::3]):
        set_switches(lom, dev, *sw)
        got = dev.evaluateFromGrids(clear, nav, states, cmd, fp, R.as_tuple(p))
        want = host.evaluate(cost, potential, states, cmd, fp, R.as_tuple(p))
        assert got[1] == want[1] == ref["summary"] and got[0].tobytes() == want[0].tobytes() == ref["picks"].tobytes()
        assert dev.records().tobytes() == host.records().tobytes() == ref["records"].tobytes()
        assert dev.stats() == dict(launches=3, waits=1)
    assert np.array_equal(clear.cost()[0], cost) and np.array_equal(nav.potential(), potential)   # the producers go on
    # without a field: no potential
    alone = reference("chain alone", table, cost, None, states, cmd, fp, p)
    got = dev.evaluateFromGrids(clear, None, states, cmd, fp, R.as_tuple(p))
    assert got[1] == alone["summary"] and got[0].tobytes() == alone["picks"].tobytes() and dev.records().tobytes() == alone["records"].tobytes()
    # the device form: planes in HBM behind a caller's event
    import torch

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        big = torch.ones(1 << 22, device="cuda:0")
        for _ in range(10):                                                       # work in front of the planes
            big = big * 1.0001 + 1.0
        t_cost = torch.from_numpy(cost).to("cuda:0", non_blocking=True) + 0
        t_pot = torch.from_numpy(potential.view(np.int32)).to("cuda:0", non_blocking=True) + 0
        ev = torch.cuda.Event()
        ev.record(stream)
    late = lom.RolloutGrid(RES, ORIGIN, w, h)
    got = late.evaluate(t_cost.data_ptr(), t_pot.data_ptr(), states, cmd, fp, R.as_tuple(p), device=True,
                        cost_event=C.c_void_p(ev.cuda_event), potential_event=C.c_void_p(ev.cuda_event))
    assert got[1] == ref["summary"] and got[0].tobytes() == ref["picks"].tobytes() and late.records().tobytes() == ref["records"].tobytes()
    torch.cuda.synchronize()
    # refused calls: the previous records stay, picks and summary are zeroed
    got = dev.evaluateFromGrids(clear, nav, states, cmd, fp, R.as_tuple(p))
    before = dev.records()
    bad_states = states.copy()
    bad_states[1, 2] = 65536
    bad_fp = fp.copy()
    bad_fp[3, 1] = 16385
    refused = [lambda: dev.evaluateFromGrids(lom.ClearanceGrid(RES, ORIGIN, w + 1, h), nav, states, cmd, fp, R.as_tuple(p)),
               lambda: dev.evaluateFromGrids(clear, lom.NavField(RES, (ORIGIN[0] + 1e-6, ORIGIN[1]), w, h), states, cmd, fp, R.as_tuple(p)),
               lambda: dev.evaluate(cost, potential, states, cmd, fp, R.as_tuple(dict(p, segments=9))),
               lambda: dev.evaluate(cost, potential, states, cmd, fp, R.as_tuple(dict(p, min_steps=81))),
               lambda: dev.evaluate(cost, potential, states, cmd, fp, R.as_tuple(dict(p, flags=2))),
               lambda: dev.evaluate(cost, potential, bad_states, cmd, fp, R.as_tuple(p)),
               lambda: dev.evaluate(cost, potential, states, cmd, bad_fp, R.as_tuple(p)),
               lambda: dev.evaluate(cost, potential, states, cmd, fp[:0], R.as_tuple(p))]
    for call in refused:
        with pytest.raises(lom.LomError) as e:
            call()
        assert e.value.code == lom.capi.ERR_ARG
        assert dev.records().tobytes() == before.tobytes() == ref["records"].tobytes()
    # commands whose shape is not (K, segments, 2) never reach the library, which would read K * segments pairs of them
    for short in (cmd[:, :1], cmd.reshape(-1)[:-2], np.zeros((len(cmd), 2, 1), np.int16), np.concatenate([cmd, cmd], axis=1)):
        with pytest.raises(ValueError):
            dev.evaluate(cost, potential, states, short, fp, R.as_tuple(p))
        assert dev.records().tobytes() == before.tobytes()
    # the C entry itself zeroes the picks and the summary of a refused call
    picks, sm = np.full(len(states), 7, lom.capi.ROLLOUT_PICK), lom.capi.RolloutSummary(1, 2, 3, 4, 5)
    st = lom.RolloutGrid._states(states)
    bad = lom.rolloutParams(R.as_tuple(dict(p, lethal_min=0)))
    rc = lom.capi.lib().lom_rollout_evaluate(dev.handle, cost.ctypes.data, None, st.ctypes.data, len(st), cmd.ctypes.data, len(cmd),
                                             np.ascontiguousarray(fp, np.int32).ctypes.data, len(fp), C.byref(bad), picks.ctypes.data, C.byref(sm))
    assert rc == lom.capi.ERR_ARG and not picks.tobytes().strip(b"\0") and sm.asdict() == dict.fromkeys(R.SUMMARY_KEYS, 0)
    # without LOM_ROLLOUT_KEEP_RECORDS there are none to read
    dev.evaluate(cost, potential, states, cmd, fp, R.as_tuple(dict(p, flags=0)))
    with pytest.raises(lom.LomError) as e:
        dev.records()
    assert e.value.code == lom.capi.ERR_STATE
    dev.clear()
    assert len(dev.records()) == 0


# ---- mirrors ---------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom, table):
    """lom::RolloutGrid of the C++ mirror leaves the bytes the Python package and the reference leave."""
    exe = cpp_program.build_with_library(tmp_path, "test_rollout_mirror.cpp")
    stdout = cpp_program.run(exe, "device", timeout=120)
    lines = stdout.rstrip("\n").split("\n")
    got_summary = [int(v) for v in lines[-3].split()]
    got_picks = np.array([int(v) for v in lines[-2].split()], np.int64).reshape(-1, 3)
    got_records = np.array([int(v) for v in lines[-1].split()], np.int64).reshape(-1, 8)
    # the same grid, planes, states, commands and footprint here (tests/cpp/test_rollout_mirror.cpp)
    w, h = 45, 37
    i = np.arange(w * h)
    plane = np.where(i % 97 == 3, 100, np.where(i % 41 == 0, -1, i % 13)).astype(np.int8).reshape(h, w)
    potential = np.where(i % 53 == 5, R.UNREACHED, (i * 7) % 3000).astype(np.uint32).reshape(h, w)
    states = [[(k * 9 + 2) * CELL + 100 * k, (k * 7 + 3) * CELL + 5, k * 9000] for k in range(5)] + [[-40000, 70000, 0]]
    cmd = np.array([[[(k * 911) % 30000 - 9000, (k * 37 + l * 500) % 1200 - 600] for l in range(2)] for k in range(70)], np.int16)
    fp = lom.rolloutFootprintRectangle(300, 200, 150, 100, True)
    p = R.params(2, 20, 100, 7, 3, 2, 1, 50, R.KEEP_RECORDS)
    ref = R.evaluate_fast(plane, potential, states, cmd, fp, table, p)
    assert got_summary == [ref["summary"][k] for k in R.SUMMARY_KEYS] and ref["summary"]["admissible"] > 20
    assert got_picks.tolist() == [[int(v) for v in e] for e in ref["picks"]]
    assert got_records.tolist() == [[int(v) for v in e] for e in ref["records"]]
