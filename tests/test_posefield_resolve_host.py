"""The pose field's re-solve without a device: the reference's incremental form (tests/posefield_resolve_ref.py) against its
full solve on every case of tests/posefield_resolve_cases.py, the least raised set against its definition, the case table
itself (no case is vacuous), the doorway, and the refusals of the library that come before any device is looked at."""
import ctypes as C
import os
import re

import numpy as np

from tests import posefield_ref as R
from tests import posefield_resolve_cases as T
from tests import posefield_resolve_ref as Q
from tests import posefield_scenes as S
from tests.conftest import ROOT

NEW_SYMBOLS = ["lom_posefield_resolve", "lom_posefield_resolve_device", "lom_posefield_resolve_from_clearance", "lom_posefield_resolve_stats"]


def test_raise_then_relax_is_the_full_solve_on_every_case():
    """dropping the impassable goal states, raising the least raised set and relaxing to the fixed point gives the full solve
    of the merged plane from the derived goal states; the raise phase keeps upper bounds only"""
    for c in T.cases():
        first, ref = T.references(c)
        P, rose = Q.raise_then_relax(first["P"], ref["L"], c["p"])
        assert P.tobytes() == ref["P"].tobytes(), c["name"]
        assert len(rose) == ref["states_raised"], c["name"]
        kept = ref["P_raised"] != Q.U
        assert (ref["P_raised"][kept].astype(np.int64) >= ref["P"][kept].astype(np.int64)).all() and (ref["P"][kept] != Q.U).all(), c["name"]
        s = ref["summary"]
        assert s["goals_used"] + s["goals_rejected"] == first["summary"]["goals_used"], c["name"]


def test_the_least_raised_set_is_the_definitions_up_to_9_x_5():
    """visiting the states in increasing P against iterating "unsafe" to a fixed point, on random planes and changes"""
    rng = np.random.default_rng(5)
    n = 0
    for w, h in ((1, 1), (2, 2), (5, 3), (9, 5), (3, 5), (9, 1)):
        for p in (T.P_NONE, T.P_BOTH, R.params(T.NAV, 0, 1, 0, T.BOTH)):
            for fp in (S.POINT, S.RECT_5x3):
                for _ in range(4):
                    kept = S.sparse(rng, w, h, 0.1)
                    new = S.sparse(rng, w, h, 0.2)
                    first = R.solve(T.geo_of(w, h), kept, p, fp, T.goals_on(kept, p, fp, 2))
                    L = R.layers(new, p, R.stencils(fp))
                    edges = R.edges_of(L, p)
                    a, b = Q.as_list(first["P"]), Q.as_list(first["P"])
                    Q.drop_impassable(a, L), Q.drop_impassable(b, L)
                    assert Q.least_raised_set(a, edges) == Q.raised_by_definition(b, edges) and a == b, (w, h, fp.shape)
                    n += 1
    assert n == 144


def test_no_case_is_vacuous():
    """the case table on the reference alone"""
    names = set()
    for c in T.cases():
        first, ref = T.references(c)
        names.add(c["name"].split("/")[-1] if c["tags"] & {"degenerate", "outside"} else "")
        if not c["tags"] & {"degenerate", "outside"}:
            assert ref["cells_changed"] > 0 and ref["states_changed"] > 0, c["name"]
        if "outside" in c["tags"]:
            assert Q.clip(c["w"], c["h"], c["window"]) is None and ref["cells_changed"] == 0, c["name"]
        if "raises" in c["tags"]:
            assert ref["states_raised"] > 0, c["name"]
        if "lowers" in c["tags"]:
            assert (ref["P"].astype(np.int64) < first["P"].astype(np.int64)).any(), c["name"]
    assert names == {"", "same_plane", "wall_to_99", "all_blocked", "window_outside"}
    for c in T.cases():
        first, ref = T.references(c)
        kind = c["name"].split("/")[-1]
        if kind == "same_plane":
            assert ref["cells_changed"] == 0 and ref["P"].tobytes() == first["P"].tobytes()
        if kind == "wall_to_99":
            assert (ref["cells_changed"], ref["states_changed"]) == (1, 0) and ref["P"].tobytes() == first["P"].tobytes()
        if kind == "all_blocked":
            assert ref["summary"]["states_reached"] == 0 and ref["summary"]["goals_used"] == 0
    assert {(c["w"], c["h"]) for c in T.cases()} == set(T.SHAPES)
    by_name = {c["name"]: T.references(c) for c in T.cases()}
    # the goal cell beside the new wall keeps the headings along the wall and loses the others ...
    s = by_name["goal_headings_rejected/both"][1]["summary"]
    assert by_name["goal_headings_rejected/both"][0]["summary"]["goals_used"] == 8 and (s["goals_used"], s["goals_rejected"]) == (2, 6)
    # ... and a heading the solve skipped is no goal once it is passable (rule c)
    first, ref = by_name["goal_heading_skipped_then_passable/both"]
    assert first["summary"]["goals_used"] == 2 and ref["summary"]["goals_used"] == 2 and ref["summary"]["goals_rejected"] == 0
    assert first["L"][2, 8, 32] == 0 and ref["L"][2, 8, 32] != 0 and 0 < ref["P"][2, 8, 32] != Q.U
    assert ref["P"][0, 8, 32] == 0 and ref["P"][4, 8, 32] == 0


def test_the_doorway():
    """one of the three door cells closes: the point still gets through at the same cost, the rectangle does not"""
    w, h = 48, 32
    plane, _ = S.doorway(w, h, 3)
    shut = T.put(plane, [(24, 17)], 100)
    counts = {}
    for name, fp in (("point", S.POINT), ("9x3", S.RECT_9x3)):
        first = R.solve(T.geo_of(w, h), plane, T.P_DOOR, fp, [(43, 16, -1)])
        ref = Q.resolve(T.geo_of(w, h), plane, shut, (24, 17, 1, 1), T.P_DOOR, fp, first)
        counts[name] = (first["summary"]["states_reached"], ref["summary"]["states_reached"], ref["states_raised"],
                        int(first["floor"][16, 5]), int(ref["floor"][16, 5]))
    print(counts)
    assert counts["point"][3] != Q.U and counts["point"][3] == counts["point"][4]
    assert counts["9x3"][3] != Q.U and counts["9x3"][4] == Q.U
    assert counts["9x3"][1] < counts["9x3"][0]


def test_new_symbols_are_declared_and_refuse_without_a_handle(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"LOM_POSE_OPT_TEST_RESOLVE_FORM\s*=\s*4", text) and lom.capi.POSE_OPT_TEST_RESOLVE_FORM == 4
    assert re.search(r"\} lom_posefield_resolve_counters;", text)
    assert C.sizeof(lom.capi.PoseFieldResolveCounters) == 56
    assert [k for k, _ in lom.capi.PoseFieldResolveCounters._fields_] == ["cells_changed", "states_changed", "states_raised", "raise_launches",
                                                                          "relax_launches", "waits", "tiles_marked"]
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for method in ("resolve", "resolveFromClearance", "resolveStats"):
        assert re.search(r"\b%s\s*\(" % method, mirror), method
        assert hasattr(lom.PoseField, method), method
    L = lom.capi.lib()
    st, sm = lom.capi.PoseFieldResolveCounters(), lom.capi.PoseFieldSummary(states_reached=7, goals_used=3)
    plane = np.zeros(4, np.int8)
    assert L.lom_posefield_resolve(None, plane.ctypes.data, None, C.byref(sm)) == lom.capi.ERR_ARG
    assert sm.asdict() == dict.fromkeys(R.SUMMARY_KEYS, 0)                 # a refusal zeroes the summary
    assert L.lom_posefield_resolve_device(None, None, None, None, None) == lom.capi.ERR_ARG
    assert L.lom_posefield_resolve_from_clearance(None, None, None, None) == lom.capi.ERR_ARG
    assert L.lom_posefield_resolve_stats(None, C.byref(st)) == lom.capi.ERR_ARG
