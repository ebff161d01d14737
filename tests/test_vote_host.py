"""Scan votes, the parts that need no GPU: the reference (tests/vote_ref.py) against the carve's reference and against
geometry, the special cases of the stop rule, the mover scene on the reference alone, the declarations, and the
refusals that touch no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import carve_ref as R
from tests import vote_ref as V
from tests import vote_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_map_carve_scans", "lom_map_scan_votes", "lom_odometry_set_rebuild_votes",
               "lom_odometry_get_rebuild_vote_stats"]


def _rays(seed, voxel, n, origin_cell=(1, -2, 0)):
    rng = np.random.default_rng(seed)
    lo, hi = R.cell_bounds(np.asarray(origin_cell, np.float64), float(np.float32(voxel)))
    origin = (lo + (hi - lo) * rng.uniform(0.1, 0.9, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = (origin + d * rng.uniform(1.5 * voxel, 18 * voxel, (n, 1))).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    return origin, pts, nrm


@pytest.mark.parametrize("voxel", [0.2, 0.5])
def test_without_clearance_the_walk_is_the_carves(voxel):
    origin, pts, nrm = _rays(7, voxel, 300)
    pc = R.params(margin=0.3 * voxel, min_range=2 * voxel, max_range=15 * voxel, min_crossings=1)
    pv = V.params(pc["margin"], pc["min_range"], pc["max_range"], 0.0, 1, 0)
    a, b = R.walk(origin, pts, voxel, pc), V.walk(origin, pts, nrm, voxel, pv)
    assert not a["error"] and not b["error"] and len(a["ray"]) > 3000
    assert np.array_equal(a["walked"], b["walked"])
    assert np.array_equal(a["ray"], b["ray"]) and np.array_equal(a["cell"], b["cell"])
    ta, tb = R.t_end_of(origin, pts, pc)[0], V.t_end_of(origin, pts, nrm, pv)[0]
    assert ta.tobytes() == tb.tobytes()


@pytest.mark.parametrize("voxel,clearance", [(0.2, 0.3), (0.5, 0.75), (0.5, 0.1)])
def test_with_a_clearance_the_walk_visits_exactly_the_cells_the_shortened_segment_meets(voxel, clearance):
    origin, pts, nrm = _rays(11 + int(clearance * 100), voxel, 150)
    p = V.params(0.3 * voxel, voxel, 15 * voxel, clearance, 1, 0)
    Vd = float(np.float32(voxel))
    w = V.walk(origin, pts, nrm, voxel, p)
    t_end, walked, L = V.t_end_of(origin, pts, nrm, p)
    assert not w["error"] and np.array_equal(w["walked"], walked)
    O = origin.astype(np.float64)
    by_plane = by_reach = skipped = 0
    for i in range(len(pts)):
        got = [tuple(c) for c in w["cell"][w["ray"] == i].tolist()]
        if not walked[i]:
            assert got == []
            skipped += 1
            continue
        D = pts[i].astype(np.float64) - O
        # the stop's geometry: at t_end the ray is `clearance` from the endpoint's plane, or margin before the reach
        dist = abs(float(np.dot(nrm[i].astype(np.float64), D))) * (1.0 - t_end[i])
        reach = (min(L[i], float(np.float32(p["max_range"]))) - float(np.float32(p["margin"]))) / L[i]
        if t_end[i] < reach:
            assert abs(dist - float(np.float32(clearance))) < 1e-9 * max(1.0, L[i])
            by_plane += 1
        else:
            assert dist >= float(np.float32(clearance)) - 1e-9 and t_end[i] == reach
            by_reach += 1
        assert len(set(got)) == len(got), i
        assert set(got) == R.cells_met_by_segment(O, D, float(t_end[i]), Vd), i
    # both stops occur (the reach only where max_range clips the ray: the margin is smaller than any clearance / c), and
    # rays too flat to walk at all
    assert by_plane > 10 and by_reach > 0 and skipped > 0


def test_special_cases_of_the_stop_rule():
    o = np.array([0.125, 0.125, 0.125], np.float32)      # (binary fractions: D = (3, 0, 0) and L = 3 exactly)
    pts = np.array([[3.125, 0.125, 0.125]] * 6, np.float32)
    nan = np.nan
    nrm = np.array([[0, 0, 0],        # a zero normal: c == 0, plane = -inf, not walked
                    [0, 1, 0],        # a ray parallel to its plane: likewise
                    [nan, 0, 0],      # a NaN normal: the comparison is false, reach stays
                    [-1, 0, 0],       # head on: plane = L - clearance
                    [-0.5, 0, 0],     # plane == reach: clearance / c = 0.25 / 0.5 = margin
                    [-0.25, 0, 0]],   # c = 0.25: plane = L - 1 < reach
                   np.float32)
    p = V.params(margin=0.5, min_range=1.0, max_range=10.0, clearance=0.25, min_free_scans=1, free_per_seen=0)
    t_end, walked, L = V.t_end_of(o, pts, nrm, p)
    assert (L == 3.0).all()
    assert walked.tolist() == [False, False, True, True, True, True]
    assert t_end[0] == -np.inf and t_end[1] == -np.inf
    assert t_end[2] == 2.5 / 3.0 and t_end[3] == 2.5 / 3.0   # reach = 2.5 < plane = 2.75
    assert t_end[4] == 2.5 / 3.0                                # plane == reach: either is the same number
    assert t_end[5] == 2.0 / 3.0
    # clearance 0: the normals play no part at all
    p0 = dict(p, clearance=0.0)
    t0, w0, _ = V.t_end_of(o, pts, nrm, p0)
    assert w0.all() and (t0 == 2.5 / 3.0).all()
    # the walk itself: the ray of case 5 ends in cell 4 (x = 2.125), the others that walk in cell 5 (x = 2.625)
    w = V.walk(o, pts, nrm, 0.5, p)
    last = [w["cell"][w["ray"] == i][-1].tolist() for i in (2, 3, 4, 5)]
    assert last == [[5, 0, 0], [5, 0, 0], [5, 0, 0], [4, 0, 0]]
    # a ray clipped at max_range with a clearance: plane is measured from the endpoint, far beyond the reach
    far = V.t_end_of(o, [[30.125, 0.125, 0.125]], [[-1, 0, 0]], p)
    assert far[1].all() and far[0][0] == (10.0 - 0.5) / 30.0


def test_votes_count_scans_not_rays():
    """two scans: the first sees through voxel (2, 0, 0) with five rays and hits it with none, the second hits it"""
    export = np.array([[1.1, 0.1, 0.1], [2.1, 0.1, 0.1]], np.float32)
    through = (np.array([[2.1, 0.02 * i, 0.1] for i in range(5)], np.float32), np.tile(np.float32([-1, 0, 0]), (5, 1)))
    onto = (np.array([[1.1, 0.1, 0.1]], np.float32), np.float32([[-1, 0, 0]]))
    ident = [0, 0, 0, 1, 0, 0, 0]
    p = V.params(0.1, 0.2, 10.0, 0.0, 1, 1)
    r = V.vote(export, 0.5, [through, onto], [0, 1], [ident, ident], p)
    # scan 0: five rays cross cell 2 (where 1.1 lies) and hit cell 4 -- one free vote, not five; scan 1 hits cell 2
    assert r["free"].tolist() == [1, 0] and r["seen"].tolist() == [1, 1]
    assert r["erase"].tolist() == [True, False] and r["stats"]["voxels_erased"] == 1   # free == free_per_seen * seen: erased
    assert r["stats"]["rays_walked"] == 6 and r["stats"]["voxels_free"] == 1 and r["stats"]["scans"] == 2
    r2 = V.vote(export, 0.5, [through, onto], [0, 1], [ident, ident], dict(p, free_per_seen=2))
    assert r2["erase"].tolist() == [False, False] and r2["stats"]["voxels_protected"] == 1  # one vote short
    r3 = V.vote(export, 0.5, [through, onto], [0, 1, 0], [ident, ident, ident], p)           # an id twice votes twice
    assert r3["free"].tolist() == [2, 0] and r3["seen"].tolist() == [1, 2]


def test_mover_scene_on_the_reference_alone():
    """The scene and parameters of tests/vote_scene.py through tests/vote_ref.py, conditions as the feature's issue sets
    them: at least 90 % of the voxels that hold only mover points erased, at most 5 % of all other voxels, and at most
    5 % of the voxels of the scene without the mover.  Figures of this reference (also in DESIGN.md 7i): 97.50 % of the
    360 mover-only voxels erased, 1.38 % of the 12,579 others, 1.42 % of the 12,778 voxels of the static scene; 53,137 of
    53,193 rays walked, 2,054,217 cells visited."""
    s = S.scene(True)
    ref = V.vote(s["export"], S.VOXEL, s["scans"], s["ids"], s["poses"], S.PARAMS)
    assert not ref["error"]
    mover_share, other_share, n_mover, n_other = S.shares(s, ref)
    s0 = S.scene(False)
    ref0 = V.vote(s0["export"], S.VOXEL, s0["scans"], s0["ids"], s0["poses"], S.PARAMS)
    static_share = float(ref0["erase"].mean())
    print(f"mover scene: {n_mover} mover-only voxels, {mover_share:.4f} erased; {n_other} others, {other_share:.4f} erased; "
          f"static scene: {len(ref0['erase'])} voxels, {static_share:.4f} erased; stats {ref['stats']}")
    assert n_mover > 100
    assert mover_share >= 0.90
    assert other_share <= 0.05
    assert static_share <= 0.05


def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"scan votes", text) and re.search(r"LOM_OPT_TEST_VOTE_SLICE_MAX\s*=\s*109", text)
    assert lom.capi.OPT_TEST_VOTE_SLICE_MAX == 109
    assert C.sizeof(lom.capi.VoteParams) == 24 and C.sizeof(lom.capi.VoteStats) == 48
    mirror = open(os.path.join(ROOT, "include", "lidar_odometry_amd.hpp")).read()
    for name in ("carveScans", "scanVotes", "setRebuildVotes", "rebuildVoteStats"):
        assert re.search(r"\b%s\s*\(" % name, mirror), name
        assert hasattr(lom.VoxelGrid, name) or hasattr(lom.LidarOdometry, name), name


def test_bad_arguments_are_refused(lom):
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    good = lom.voteParams(S.PARAMS)
    st = lom.capi.VoteStats()
    st.scans = 7
    assert L.lom_map_carve_scans(None, None, None, None, 0, C.byref(good), C.byref(st)) == ERR_ARG and st.scans == 0
    assert L.lom_map_scan_votes(None, None, None, None, 0, C.byref(good), None, None, 0) == ERR_ARG
    assert L.lom_odometry_set_rebuild_votes(None, C.byref(good)) == ERR_ARG
    assert L.lom_odometry_set_rebuild_votes(None, None) == ERR_ARG
    assert L.lom_odometry_get_rebuild_vote_stats(None, C.byref(st)) == ERR_ARG
    with pytest.raises(TypeError):
        lom.voteParams(dict(margin=0.3))  # no defaults: all six fields or none
    assert lom.voteParams((0.4, 4.0, 60.0, 0.75, 3, 2)).free_per_seen == 2
