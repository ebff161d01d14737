"""Call order around the cleanup scan that runs behind an align.

lom_map_radius_cleanup_after_align arms the next align to enqueue the scan of the radius cleanup that follows it; the
scan leaves keep[] / newid[] in the map's shared scratch (S_FLAG / S_RANK, csrc/map_internal.hpp) and its give-up word
where lom_map_status looks for calls that gave up.  Between the align and the cleanup the caller may do anything the
public API offers.  Whatever it does, the map must stay the oracle's, lom_map_status must not report a call nobody
made, and the calls that neither change the map nor write that scratch must leave the scan takeable.

Bars as tests/test_gpu_parity.py: sizes, exports and searches bit-exact against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from tests import carve_ref, scenes
from tests.test_gpu_parity import _assert_same_map, _assert_same_pairs

pytestmark = pytest.mark.gpu

VOXEL, CAP, RADIUS = 0.5, 20, 6.0
GUESS = ((0.05, -0.02, 0.0), scenes.angle_axis_q(0.01, (0, 0, 1)))
CARVE = carve_ref.params(margin=0.25, min_range=0.5, max_range=6.0, min_crossings=1)
VOTE = dict(margin=0.3, min_range=0.5, max_range=8.0, clearance=0.4, min_free_scans=1, free_per_seen=1)


@pytest.fixture(autouse=True, params=["product", "counted"])
def search_mode(request, monkeypatch):
    """Both search modes, as tests/test_gpu_parity.py: the handles as a caller gets them, and LOM_COUNT_CANDIDATES=1."""
    monkeypatch.setenv("LOM_COUNT_CANDIDATES", "1" if request.param == "counted" else "0")
    return request.param


@pytest.fixture(scope="module")
def sm(oracle):
    case = scenes.small_synth_case()
    og = oracle.VoxelGrid(VOXEL, CAP)
    og.addCloud(case["map_xyz"], case["map_nrm"])
    case["n_vox"] = og.size()
    rng = np.random.default_rng(5)
    case["queries"] = np.ascontiguousarray(case["map_xyz"][rng.choice(len(case["map_xyz"]), 1500, replace=False)] + np.float32(0.02))
    return case


class Pair:
    """a device map beside the oracle's, filled and with the cleanup's scratch sized (a scan behind an align does not
    allocate), and one matcher per side"""

    def __init__(self, lom, oracle, sm):
        self.lom, self.O, self.sm = lom, oracle, sm
        self.g, self.og = lom.VoxelGrid(VOXEL, CAP), oracle.VoxelGrid(VOXEL, CAP)
        self.g.addCloud(sm["map_xyz"], sm["map_nrm"])
        self.og.addCloud(sm["map_xyz"], sm["map_nrm"])
        self.g.radiusCleanup((0, 0, 0), 1e6)
        self.m, self.om = lom.CloudMatcher(), oracle.CloudMatcher()
        self.L = lom.capi.lib()

    def counter(self, which):
        return self.g.debugCounter(which)

    def align(self, arm=None, give_up=False):
        """both sides from GUESS; the device's translation, the centre of the cleanup that follows on both sides"""
        if arm is not None:
            self.g.radiusCleanupAfterAlign(arm)
        if give_up:
            self.g.setOption(self.lom.capi.OPT_TEST_GRID_GIVE_UP, 1)
        p = self.m.align(self.g, self.sm["scan"], self.lom.Pose3D(*GUESS))
        self.om.align(self.og, self.sm["scan"], self.O.Pose3D(*GUESS))
        assert self.m.stats["outer_iterations"] == self.om.stats["outer_iterations"]
        return np.asarray(p.translation, np.float32)

    def cleanup(self, centre, radius):
        self.g.radiusCleanup(centre, radius)
        self.og.radiusCleanup(centre, radius)

    def add(self, xyz, nrm):
        self.g.addCloud(xyz, nrm)
        self.og.addCloud(xyz, nrm)

    def status(self):
        return self.L.lom_map_status(self.g.handle)

    def carve(self, origin, pts):
        """carveRays on the device; the oracle's map rebuilt from what the carve's definition (tests/carve_ref.py) keeps"""
        xyz, nrm = self.og.getCloud()
        ref = carve_ref.carve(xyz, VOXEL, origin, pts, CARVE)
        assert not ref["error"]
        st = self.g.carveRays(origin, pts, CARVE)
        assert st == ref["stats"]
        self.og = carve_ref.regrow(self.O, VOXEL, CAP, xyz[ref["point_keep"]], nrm[ref["point_keep"]])

    def same(self):
        _assert_same_map(self.g, self.og)

    def goes_on(self):
        """the map goes on as the oracle's: an insert into erased and kept voxels, exports, a search"""
        sm = self.sm
        self.add(sm["map_xyz"][:3000], sm["map_nrm"][:3000])
        self.same()
        _assert_same_pairs(self.g.findMatchingPairs(sm["queries"], self.lom.Pose3D(), 0.3),
                           self.og.findMatchingPairs(sm["queries"], self.O.Pose3D(), 0.3))


# ---- A1: one call between the align and the cleanup -------------------------------------------------------------------
def _upload(pair, n=100):
    dx = C.c_void_p()
    xyz = np.ascontiguousarray(pair.sm["scan"][:n])
    pair.lom.capi.check(pair.L.lom_upload_points(pair.g.handle, xyz.ctypes.data, None, n, 12, C.byref(dx), None), pair.g.handle)
    assert dx.value
    return dx, n


def _transform(pair):
    dx, n = _upload(pair)
    out = C.c_void_p()
    pose = pair.lom.Pose3D(*GUESS)._c()
    pair.lom.capi.check(pair.L.lom_transform_points_device(pair.g.handle, C.byref(pose), dx, None, n, 12, C.byref(out), None),
                        pair.g.handle)
    assert out.value


def _scan_votes(pair):
    a = pair.lom.ScanArchive()
    scan = pair.sm["scan"]
    nrm = np.tile(np.float32([0, 0, 1]), (len(scan), 1))
    for _ in range(2):
        a.add(scan[:500], nrm[:500])
    poses = np.array([[0, 0, 0, 1, 0, 0, 0], [0.1, 0, 0, 1, 0, 0, 0]], np.float64)
    free, seen = pair.g.scanVotes(a, [0, 1], poses, VOTE)
    assert len(free) == pair.g.size() and seen.any()


def _scan_context_align(pair):
    ctx = pair.lom.ScanContext(pair.g)
    p = pair.lom.CloudMatcher().align(ctx, pair.sm["scan"], pair.lom.Pose3D(*GUESS))
    assert np.isfinite(p.translation).all()
    ctx.close()  # (nobody changes the grid while contexts are in use)


def _carve_counts(pair):
    cross, _ = pair.g.carveCounts((0.0, 0.0, 0.0), pair.sm["scan"][:64], CARVE)  # 64 rays from inside the cloud
    assert len(cross) == pair.g.size() and cross.any()


def _poses3(pair):
    return [pair.lom.Pose3D((0.01 * i, 0.0, 0.0)) for i in range(3)]


# name -> (the call, the rise of COUNTER_CLEANUPS_BEHIND_ALIGN across the cleanup: None = not asserted).
# The issue sets 1 for nothing / size / quality / qualityBatch and leaves the four export forms open (they write counts
# and offsets over keep / newid, so the scan is dropped or given scratch of its own).  The others are derived from the
# code: none of them changes the map (call_seq, mutations, n_vox stay) and none is handed S_FLAG / S_RANK --
#   findMatchingPairs / a second align / an align on a scan context: the scan buffers and the align state only;
#   carveCounts / scanVotes: slots and buffers of their own (S_CARVE_*, the vote buffers), nothing is erased;
#   lom_upload_points / lom_transform_points_device: S_IN_XYZ only;
#   lom_map_status: reads the status words;
#   a second align that is not armed enqueues no scan, so the first one's stays in flight --
# so the scan is still the one made for this cleanup on this map: 1.
BETWEEN = {
    "nothing": (lambda p: None, 1),
    "getCloud": (lambda p: p.g.getCloud(), None),
    "getCloudWithoutNormals": (lambda p: p.g.getCloudWithoutNormals(), None),
    "getSparseCloudWithoutNormals": (lambda p: p.g.getSparseCloudWithoutNormals(), None),
    "pointCount": (lambda p: p.g.pointCount(), None),
    "size": (lambda p: p.g.size(), 1),
    "findMatchingPairs": (lambda p: p.g.findMatchingPairs(p.sm["queries"], p.lom.Pose3D(), 0.3), 1),
    "quality": (lambda p: p.g.quality(p.sm["scan"], p.lom.Pose3D(*GUESS)), 1),
    "qualityBatch": (lambda p: p.g.qualityBatch(p.sm["scan"], _poses3(p)), 1),
    "carveCounts": (_carve_counts, 1),
    "scanVotes": (_scan_votes, 1),
    "upload_points": (_upload, 1),
    "transform_points_device": (_transform, 1),
    "second_align_not_armed": (lambda p: p.m.align(p.g, p.sm["scan"], p.lom.Pose3D(*GUESS)), 1),
    "map_status": (lambda p: p.status(), 1),
    "scan_context_align": (_scan_context_align, 1),
    "two_exports": (lambda p: (p.g.getSparseCloudWithoutNormals(), p.g.getCloud()), None),
}


def _one_call_between(pair, between):
    call, rise = BETWEEN[between]
    taken = pair.lom.capi.COUNTER_CLEANUPS_BEHIND_ALIGN
    before_vox = pair.g.size()
    centre = pair.align(arm=RADIUS)
    call(pair)
    before = pair.counter(taken)
    pair.cleanup(centre, RADIUS)
    if rise is not None:
        assert pair.counter(taken) - before == rise, between
    assert pair.g.size() < before_vox, "the cleanup was meant to erase voxels"
    pair.same()
    assert pair.status() == 0
    pair.goes_on()


@pytest.mark.parametrize("between", list(BETWEEN))
def test_one_call_between_align_and_cleanup(lom, oracle, sm, between):
    pair = Pair(lom, oracle, sm)
    assert pair.g.size() == sm["n_vox"]
    _one_call_between(pair, between)


# ---- A3: the same with empty slabs in place ---------------------------------------------------------------------------
@pytest.mark.parametrize("between", ["getCloud", "pointCount", "carveCounts", "nothing"])
def test_one_call_between_with_holes_in_place(lom, oracle, sm, between):
    """An earlier cleanup that erases fewer than a quarter of the slabs leaves them in place, empty.  Their export count is
    0: export counts read as keep flags erase the holes again and keep everything else -- another wrong set than on a
    map without holes."""
    pair = Pair(lom, oracle, sm)
    pair.cleanup((0.0, 0.0, 0.0), 36.0)
    erased = sm["n_vox"] - pair.g.size()
    assert 0 < erased * 4 <= sm["n_vox"], erased
    assert pair.counter(lom.capi.COUNTER_EMPTY_SLABS) == erased
    pair.same()
    _one_call_between(pair, between)


# ---- A2: a scan that gave up and is not used --------------------------------------------------------------------------
def _other_centre(pair, centre):
    pair.cleanup(centre + np.float32(1e-3), RADIUS)


def _other_radius(pair, centre):
    pair.cleanup(centre, 5.0)


def _insert_then_cleanup(pair, centre):
    pair.add(pair.sm["map_xyz"][:50] + np.float32(0.01), pair.sm["map_nrm"][:50])
    pair.cleanup(centre, RADIUS)


def _export_then_cleanup(pair, centre):
    pair.g.getCloud()
    pair.cleanup(centre, RADIUS)


def _carve_then_cleanup(pair, centre):
    pair.carve((0.0, 0.0, 0.0), pair.sm["scan"][:64])
    pair.cleanup(centre, RADIUS)


def _second_armed_align_taken(pair, centre):
    pair.cleanup(pair.align(arm=RADIUS), RADIUS)


def _second_align_no_cleanup(pair, centre):
    pair.align()


# name -> (what follows the align whose scan gave up, a cleanup is part of it, rise of COUNTER_CLEANUPS_BEHIND_ALIGN)
AFTER_GIVE_UP = {
    "other_centre": (_other_centre, True, 0),
    "other_radius": (_other_radius, True, 0),
    "insert_then_cleanup": (_insert_then_cleanup, True, 0),
    "getCloud_then_cleanup": (_export_then_cleanup, True, None),  # (dropped, or scratch of its own: the fix's choice)
    "carveRays_then_cleanup": (_carve_then_cleanup, True, 0),
    "second_armed_align_taken": (_second_armed_align_taken, True, 1),  # (the second scan: it did not give up)
    "second_align_not_armed_no_cleanup": (_second_align_no_cleanup, False, 0),
    "nothing": (lambda pair, centre: None, False, 0),
}


@pytest.mark.parametrize("then", list(AFTER_GIVE_UP))
def test_scan_that_gave_up_and_is_not_used(lom, oracle, sm, then):
    """LOM_OPT_TEST_GRID_GIVE_UP = 1: the workgroups of the scan behind the align return at once with the give-up word
    set (the one-shot hook: nothing waits).  The scan was no call of the user's: unless a cleanup takes it -- and redoes it
    -- nobody hears of it."""
    follow, cleans, rise = AFTER_GIVE_UP[then]
    pair = Pair(lom, oracle, sm)
    taken, redos = lom.capi.COUNTER_CLEANUPS_BEHIND_ALIGN, lom.capi.COUNTER_GRID_REDOS
    t0, r0 = pair.counter(taken), pair.counter(redos)
    centre = pair.align(arm=RADIUS, give_up=True)
    follow(pair, centre)
    assert pair.status() == 0
    if rise is not None:
        assert pair.counter(taken) - t0 == rise
    # redone only where a scan that gave up was taken: the one forced give-up of this test, behind the first align
    gave_up_taken = 1 if then == "getCloud_then_cleanup" and pair.counter(taken) - t0 == 1 else 0
    assert pair.counter(redos) - r0 == gave_up_taken
    if cleans:
        assert pair.g.size() < sm["n_vox"]
    pair.same()
    pair.goes_on()  # (an addCloud that succeeds, where no cleanup was part of the case)
    assert pair.status() == 0
