"""Scan votes on the device against tests/vote_ref.py: free and seen per live voxel exactly equal, and after
carveScans the size, the full export (points and normals, byte for byte) and every stats field exactly equal."""
import numpy as np
import pytest

from tests import assemble_ref as A
from tests import carve_ref as R
from tests import cpp_program
from tests import scenes
from tests import vote_ref as V
from tests import vote_scene as S
from tests.test_carve_gpu import Pair, lattice_points, room_points

pytestmark = pytest.mark.gpu

H = np.array([4.5, 3.5, 1.7])  # half extents of the room of tests/test_carve_gpu.py
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
P1 = V.params(margin=0.3, min_range=0.5, max_range=8.0, clearance=0.4, min_free_scans=1, free_per_seen=1)


# ---- scans ----------------------------------------------------------------------------------------------------------------
def pose_in_room(rng, turn=0.6):
    """an origin well inside the room and a rotation of up to `turn` about a random axis, quaternion not normalised"""
    t = rng.uniform(-1, 1, 3) * (H - 1.2)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-turn, turn)
    q = np.r_[np.cos(ang / 2), np.sin(ang / 2) * axis] * rng.uniform(0.5, 2.0)
    return np.r_[t, q]


def room_scan(rng, n, pose, extra=None):
    """n points on the room's walls with the walls' inward normals (and `extra` world points, normals towards the
    origin), in the sensor frame of `pose`: what an archive holds"""
    face = rng.integers(0, 6, n)
    w = rng.uniform(-1, 1, (n, 3)) * H
    side = np.where(face % 2 == 0, -1.0, 1.0)
    w[np.arange(n), face // 2] = side * H[face // 2] + rng.normal(0, 0.01, n)
    nw = np.zeros((n, 3))
    nw[np.arange(n), face // 2] = -side
    if extra is not None and len(extra):
        d = pose[:3] - extra
        w, nw = np.concatenate([w, extra]), np.concatenate([nw, d / np.linalg.norm(d, axis=1)[:, None]])
    Rm = A.rotation_matrix(pose)
    return ((w - pose[:3]) @ Rm).astype(np.float32), (nw @ Rm).astype(np.float32)


class Archive:
    """a device archive and the host copy of its scans for the reference"""

    def __init__(self, lom, scans=()):
        self.dev, self.scans = lom.ScanArchive(), []
        for x, n in scans:
            self.add(x, n)

    def add(self, x, n):
        x, n = np.ascontiguousarray(x, np.float32).reshape(-1, 3), np.ascontiguousarray(n, np.float32).reshape(-1, 3)
        assert self.dev.add(x, n) == len(self.scans)
        self.scans.append((x, n))


def room_archive(lom, sizes, seed, ghosts=None, turn=0.6):
    rng = np.random.default_rng(seed)
    poses = np.stack([pose_in_room(rng, turn) for _ in sizes])
    scans = []
    for k, n in enumerate(sizes):
        extra = ghosts[rng.permutation(len(ghosts))[:len(ghosts) // 3]] if (ghosts is not None and k % 2 == 1) else None
        scans.append(room_scan(rng, n, poses[k], extra))
    return Archive(lom, scans), poses


class VPair(Pair):
    def ref(self, a, ids, poses, p):
        return V.vote(self.xyz, self.voxel, a.scans, ids, poses, p)

    def check_votes(self, a, ids, poses, p):
        ref = self.ref(a, ids, poses, p)
        assert not ref["error"]
        free, seen = self.g.scanVotes(a.dev, ids, poses, p)
        assert len(free) == len(ref["free"]) == self.g.size()
        assert np.array_equal(free, ref["free"]), np.flatnonzero(free != ref["free"])[:10]
        assert np.array_equal(seen, ref["seen"]), np.flatnonzero(seen != ref["seen"])[:10]
        self.check_export()
        return ref

    def check_carve(self, a, ids, poses, p):
        ref = self.ref(a, ids, poses, p)
        assert not ref["error"]
        st = self.g.carveScans(a.dev, ids, poses, p)
        print("votes", st)
        assert st == ref["stats"]
        self.xyz, self.nrm = self.xyz[ref["point_keep"]], self.nrm[ref["point_keep"]]
        self.check_export()
        assert self.g.pointCount() == len(self.xyz)
        return ref


def room_pair(lom, oracle, seed=3):
    xyz, nrm = room_points(seed=seed)
    return VPair(lom, oracle, 0.5, 6, xyz, nrm)


def ghosts_of(pair):
    inside = np.all(np.abs(pair.xyz) < H - 0.7, axis=1)
    return pair.xyz[inside].astype(np.float64)


@pytest.fixture(scope="module")
def room(lom, oracle):
    return room_pair(lom, oracle)


@pytest.fixture(scope="module")
def lattice(lom, oracle):
    xyz, nrm = lattice_points(0.5, 6)
    return VPair(lom, oracle, 0.5, 4, xyz, nrm)


# ---- 1, 2: the votes -------------------------------------------------------------------------------------------------------
def test_votes_of_ragged_scans(lom, oracle):
    pair = room_pair(lom, oracle)
    a, poses = room_archive(lom, [40, 700, 0, 257, 300], seed=71, ghosts=ghosts_of(pair))
    ids = np.arange(5)
    p = V.params(0.3, 0.5, 8.0, 0.4, 2, 1)
    ref = pair.check_votes(a, ids, poses, p)                     # nothing erased: the export is unchanged
    assert ref["free"].max() >= 3 and ref["seen"].max() >= 3 and ((ref["free"] > 0) & (ref["seen"] > 0)).any()
    assert ref["stats"]["voxels_free"] > 50 and ref["stats"]["rays_walked"] > 1000
    pair.check_carve(a, ids, poses, p)                           # the stats, field by field


def test_against_the_librarys_own_carve(lom, room):
    """clearance = 0: the votes are K calls of lom_map_carve_counts put together"""
    a, poses = room_archive(lom, [300, 0, 511, 64, 700], seed=72, ghosts=ghosts_of(room))
    p = V.params(0.3, 0.5, 6.0, 0.0, 1, 0)
    pc = R.params(0.3, 0.5, 6.0, 1)
    free, seen = np.zeros(room.g.size(), np.int64), np.zeros(room.g.size(), np.int64)
    for k in range(5):
        pts, _ = A.transform(poses[k], *a.scans[k])
        cross, hit = room.g.carveCounts(V.origin_of(poses[k]), pts, pc)
        seen += hit > 0
        free += (cross > 0) & (hit == 0)
    got_free, got_seen = room.g.scanVotes(a.dev, np.arange(5), poses, p)
    assert np.array_equal(got_free, free) and np.array_equal(got_seen, seen)
    assert free.max() >= 3 and seen.max() >= 2
    room.check_export()


# ---- 3: slices ---------------------------------------------------------------------------------------------------------------
def test_slices(lom, room):
    """70 scans of 40 rays, every id twice with two poses: one scan per launch, seven, and 64 + 6 give the same counts"""
    L = lom.capi.lib()
    a, _ = room_archive(lom, [40] * 35, seed=73, ghosts=ghosts_of(room))
    rng = np.random.default_rng(74)
    ids = np.r_[np.arange(35), np.arange(35)[::-1]]
    poses = np.stack([pose_in_room(rng) for _ in range(70)])
    ref = room.check_votes(a, ids, poses, P1)
    assert ref["seen"].max() > 1 and ref["free"].max() > 10
    out = {}
    try:
        for cap in (1, 7, 0):
            lom.capi.check(L.lom_map_set_option(room.g.handle, lom.capi.OPT_TEST_VOTE_SLICE_MAX, cap), room.g.handle)
            out[cap] = room.g.scanVotes(a.dev, ids, poses, P1)
    finally:
        L.lom_map_set_option(room.g.handle, lom.capi.OPT_TEST_VOTE_SLICE_MAX, 0)
    for cap in (1, 7, 0):
        assert np.array_equal(out[cap][0], ref["free"]) and np.array_equal(out[cap][1], ref["seen"]), cap
    assert L.lom_map_set_option(room.g.handle, lom.capi.OPT_TEST_VOTE_SLICE_MAX, 65) == lom.capi.ERR_ARG
    for K in (64, 65):
        room.check_votes(a, ids[:K], poses[:K], P1)


# ---- 4: the stop rule ------------------------------------------------------------------------------------------------------
def test_stop_rule_on_the_lattice(lattice):
    """The lattice has a voxel in every cell, so free / seen show every cell a walk visits.  One ray per scan: chosen
    incidences, the four special cases of the header's step 4, a ray clipped at max_range, and an endpoint nearer than
    min_range, which still hits."""
    nan = np.nan
    o = [0.125, 0.125, 0.125]
    rays = [  # (endpoint, normal), sensor frame = map frame moved by o
        ([2.5, 0.0, 0.0], [-1, 0, 0]),        # head on: plane = L - clearance
        ([2.5, 0.0, 0.0], [-0.5, 0, 0]),      # plane == reach
        ([2.5, 0.0, 0.0], [-0.25, 0, 0]),     # the plane stops it first
        ([2.5, 0.0, 0.0], [0, 0, 0]),         # a zero normal: not walked
        ([2.5, 0.0, 0.0], [0, 1, 0]),         # parallel to its plane: not walked
        ([2.5, 0.0, 0.0], [nan, 0, 0]),       # a NaN normal: reach
        ([2.0, 1.5, -1.0], [-0.6, 0, 0.8]),   # oblique
        ([-2.0, 2.2, 0.4], [0.1, -0.2, 0.97]),  # grazing: c is small, the walk ends early
        ([0.0, -3.0, 0.0], [0, 1, 0]),        # clipped at max_range = 2.75 (L = 3)
        ([0.25, 0.0, 0.0], [-1, 0, 0]),       # L < min_range: no walk, but a hit
    ]
    a = Archive(lattice.lom, [(np.float32([e]), np.float32([n])) for e, n in rays])
    poses = np.tile(np.r_[o, 1, 0, 0, 0], (len(rays), 1))
    p = V.params(margin=0.5, min_range=0.5, max_range=2.75, clearance=0.25, min_free_scans=1, free_per_seen=0)
    walked = []
    for k in range(len(rays)):  # every ray on its own, then all together
        ref = lattice.check_votes(a, [k], poses[k:k + 1], p)
        walked.append(ref["stats"]["rays_walked"])
        assert ref["seen"].sum() == 1
    assert walked == [1, 1, 1, 0, 0, 1, 1, 1, 1, 0]
    ends = [V.walk(o, [e], [n], 0.5, p)["cell"][-1].tolist() for e, n in rays[:3]]
    assert ends == [[4, 0, 0], [4, 0, 0], [3, 0, 0]]  # x = 0.125 + 2.0 resp. 0.125 + 1.5
    ref = lattice.check_votes(a, np.arange(len(rays)), poses, p)
    assert ref["free"].max() >= 5 and ref["stats"]["rays_skipped"] == 3
    ref0 = lattice.check_votes(a, np.arange(len(rays)), poses, dict(p, clearance=0.0))  # no such stop: the normals play no part
    assert ref0["stats"]["rays_walked"] == 9 and ref0["stats"]["cells_visited"] > ref["stats"]["cells_visited"]


# ---- 5: thresholds ---------------------------------------------------------------------------------------------------------
def make_threshold_scene(lom, oracle):
    pair = room_pair(lom, oracle, seed=8)
    a, poses = room_archive(lom, [300] * 12, seed=75, ghosts=ghosts_of(pair))
    xyz, nrm = room_points(seed=8)
    return a, poses, xyz, nrm


@pytest.fixture(scope="module")
def threshold_scene(lom, oracle):
    return make_threshold_scene(lom, oracle)


@pytest.mark.parametrize("free_per_seen", [0, 1, 2])
@pytest.mark.parametrize("min_free_scans", [1, 2, 3])
def test_thresholds(lom, oracle, threshold_scene, min_free_scans, free_per_seen):
    a, poses, xyz, nrm = threshold_scene
    pair = VPair(lom, oracle, 0.5, 6, xyz, nrm)
    p = V.params(0.3, 0.5, 8.0, 0.4, min_free_scans, free_per_seen)
    ref = pair.check_carve(a, np.arange(12), poses, p)
    f, s = ref["free"].astype(np.int64), ref["seen"].astype(np.int64)
    assert ref["stats"]["voxels_erased"] > 0
    if free_per_seen:
        on_the_line = (s > 0) & (f == free_per_seen * s) & (f >= min_free_scans)
        one_short = (s > 0) & (f == free_per_seen * s - 1) & (f >= min_free_scans)
        assert on_the_line.any() and ref["erase"][on_the_line].all()       # free == free_per_seen * seen: erased
        assert one_short.any() and not ref["erase"][one_short].any()       # one vote short: kept
        assert ref["stats"]["voxels_protected"] >= int(one_short.sum())
    else:
        assert ((s > 0) & ref["erase"]).any()                               # the ratio is off: a seen voxel goes too
    assert (f < min_free_scans).any() and not ref["erase"][f < min_free_scans].any()   # too few free votes: kept


# ---- 6: the erase ----------------------------------------------------------------------------------------------------------
def test_in_place_erase_and_reinsert(lom, oracle):
    xyz, nrm = room_points(seed=12)
    pair = VPair(lom, oracle, 0.5, 6, xyz, nrm)
    nv = pair.g.size()
    a, poses = room_archive(lom, [300] * 6, seed=76, ghosts=ghosts_of(pair))
    ref = pair.check_carve(a, np.arange(6), poses, V.params(0.3, 0.5, 8.0, 0.4, 3, 2))
    erased = ref["stats"]["voxels_erased"]
    assert 0 < erased * 4 <= nv
    assert pair.g.debugCounter(lom.capi.COUNTER_EMPTY_SLABS) == erased   # in place: the slabs stay, empty
    # votes over a map with those holes
    a2, poses2 = room_archive(lom, [200] * 4, seed=77)
    pair.check_votes(a2, np.arange(4), poses2, P1)
    pair.check_carve(a2, np.arange(4), poses2, V.params(0.3, 0.5, 8.0, 0.4, 2, 1))
    # re-insert: a point into an erased voxel and one elsewhere; the erased voxel comes back at the end of the creation order
    gone = xyz[~np.isin(R.pack(R.map_index(xyz, 0.5)[0]), R.voxels_of_export(pair.xyz, 0.5)[0])]
    assert len(gone)
    new_x = np.concatenate([gone[:3], pair.xyz[:2]]).astype(np.float32)
    new_n = np.ones_like(new_x)
    og = pair.oracle()
    og.addCloud(new_x, new_n)
    pair.g.addCloud(new_x, new_n)
    pair.take(og)
    pair.check_export()
    assert R.pack(R.map_index(pair.xyz[-1:], 0.5)[0])[0] in set(R.pack(R.map_index(gone[:3], 0.5)[0]).tolist())


def test_compaction_and_dense_switch(lom, oracle, monkeypatch):
    """the lattice has no free space: every voxel two scans see through and none sees goes, far more than a quarter"""
    xyz, nrm = lattice_points(0.5, 5)
    pair = VPair(lom, oracle, 0.5, 4, xyz, nrm)
    nv = pair.g.size()
    rng = np.random.default_rng(21)
    scans, poses = [], []
    for k in range(4):
        pts = rng.uniform(-2.7, 2.7, (400, 3))
        pts[np.arange(400), rng.integers(0, 3, 400)] = rng.choice([-2.7, 2.7], 400)  # endpoints in the outermost cells only
        o = rng.uniform(-0.4, 0.4, 3)
        d = pts - o
        scans.append((d.astype(np.float32), (-d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)))
        poses.append(np.r_[o, 1, 0, 0, 0])
    a = Archive(lom, scans)
    p = V.params(0.3, 0.5, 6.0, 0.2, 2, 1)
    ref = pair.check_carve(a, np.arange(4), np.stack(poses), p)
    assert ref["stats"]["voxels_erased"] * 4 > nv
    assert pair.g.debugCounter(lom.capi.COUNTER_EMPTY_SLABS) == 0
    pair.check_votes(a, np.arange(4), np.stack(poses), P1)  # the rebuilt table
    # LOM_DENSE_CLEANUP: a few holes are closed at once as well
    monkeypatch.setenv("LOM_DENSE_CLEANUP", "1")
    x2, n2 = room_points(seed=12)
    dense = VPair(lom, oracle, 0.5, 6, x2, n2)
    a2, poses2 = room_archive(lom, [300] * 6, seed=76, ghosts=ghosts_of(dense))
    ref = dense.check_carve(a2, np.arange(6), poses2, V.params(0.3, 0.5, 8.0, 0.4, 3, 2))
    assert 0 < ref["stats"]["voxels_erased"] * 4 <= len(ref["free"])
    assert dense.g.debugCounter(lom.capi.COUNTER_EMPTY_SLABS) == 0


# ---- 7: errors -------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_map_alone(lom, room):
    """(A walk that leaves the index range with its origin and its endpoint inside cannot be built: the range is a box
    and the segment lies in it.  The origin and the endpoint out of range are what reaches the error word.)"""
    import ctypes as C
    L = lom.capi.lib()
    a, poses = room_archive(lom, [100, 64, 30], seed=78)
    a.add(np.float32([[400.0, 1.0, 0.5], [1.0, 1.0, 0.5]]), np.float32([[-1, 0, 0], [-1, 0, 0]]))   # scan 3: a far point
    bad = a.scans[1][0].copy()
    bad[17, 1] = np.nan
    ws, dx, dn = lom.VoxelGrid(0.5, 1), C.c_void_p(), C.c_void_p()     # the cloud in HBM: another handle's staging buffers
    lom.capi.check(L.lom_upload_points(ws.handle, bad.ctypes.data, a.scans[1][1].ctypes.data, 64, 12, C.byref(dx), C.byref(dn)),
                   ws.handle)
    lom.capi.check(L.lom_map_status(ws.handle), ws.handle)             # (waits for that handle's copies)
    assert a.dev.addDevice(dx, dn, 64) == 4                                                        # scan 4: a NaN inside
    a.scans.append((bad, a.scans[1][1]))
    ids3 = np.arange(3)
    far = np.r_[524000.0, 0, 0, 1, 0, 0, 0]       # index 1,048,000: inside; + 400 m: outside
    out = np.r_[0, -524288.0, 0, 1, 0, 0, 0]      # the origin itself outside
    huge = np.r_[0, 0, 1e300, 1, 0, 0, 0]         # rounds to +inf in f32

    def refused(code, ids, p, prm=P1):
        for call in (lambda: room.g.carveScans(a.dev, ids, p, prm), lambda: room.g.scanVotes(a.dev, ids, p, prm)):
            with pytest.raises(lom.LomError) as e:
                call()
            assert e.value.code == code, (ids, e.value)
        room.check_export()

    refused(lom.capi.ERR_RANGE, [0, 4, 2], poses)                                   # the NaN, in the middle scan
    assert V.vote(room.xyz, 0.5, a.scans, [0, 4, 2], poses, P1)["error"]
    refused(lom.capi.ERR_RANGE, [0, 3], np.stack([poses[0], far]))                  # an endpoint thrown out of range
    assert V.vote(room.xyz, 0.5, a.scans, [0, 3], np.stack([poses[0], far]), P1)["error"]
    assert not V.vote(room.xyz, 0.5, a.scans, [0, 3], poses[:2], P1)["error"]
    refused(lom.capi.ERR_RANGE, [0, 1], np.stack([poses[0], out]))                  # an origin out of range
    refused(lom.capi.ERR_RANGE, [0, 1], np.stack([poses[0], huge]))
    assert V.vote(room.xyz, 0.5, a.scans, [0, 1], np.stack([poses[0], out]), P1)["error"]
    for change in (dict(margin=-0.1), dict(min_range=0.0), dict(max_range=0.4), dict(clearance=-1.0), dict(clearance=np.nan),
                   dict(max_range=np.inf), dict(min_free_scans=0)):
        refused(lom.capi.ERR_ARG, ids3, poses, dict(P1, **change))                  # bad params
    for ids, p in (([5], IDENT[None]), ([-1], IDENT[None]), ([0], np.array([[0, 0, 0, 0, 0, 0, 0.0]])),
                   ([0, 1], np.array([IDENT, [np.nan, 0, 0, 1, 0, 0, 0]]))):
        refused(lom.capi.ERR_ARG, ids, p)                                           # a bad id, a bad pose
    ctx = lom.ScanContext(room.g)                                                   # a scan context
    prm = lom.voteParams(P1)
    ids64, p64 = np.zeros(1, np.int64), np.zeros(1, lom.capi.GRAPH_POSE)
    p64["q_wxyz"][0, 0] = 1.0
    st = lom.capi.VoteStats()
    assert L.lom_map_carve_scans(ctx.handle, a.dev.handle, ids64.ctypes.data, p64.ctypes.data, 1, C.byref(prm), C.byref(st)) == lom.capi.ERR_ARG
    assert st.asdict() == lom.capi.VoteStats().asdict()
    assert L.lom_map_scan_votes(ctx.handle, a.dev.handle, ids64.ctypes.data, p64.ctypes.data, 1, C.byref(prm), None, None, 0) == lom.capi.ERR_ARG
    assert L.lom_map_carve_scans(room.g.handle, a.dev.handle, None, p64.ctypes.data, 1, C.byref(prm), None) == lom.capi.ERR_ARG
    assert L.lom_map_carve_scans(room.g.handle, a.dev.handle, ids64.ctypes.data, p64.ctypes.data, 1, None, None) == lom.capi.ERR_ARG
    room.check_export()
    # nothing to do: count == 0 and only empty scans
    a.add(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    st = room.g.carveScans(a.dev, [], np.empty((0, 7)), P1)
    assert st["scans"] == 0 and st["voxels_erased"] == 0
    st = room.g.carveScans(a.dev, [5, 5], np.stack([IDENT, IDENT]), P1)
    assert st == dict(scans=2, rays_walked=0, rays_skipped=0, cells_visited=0, voxels_free=0, voxels_protected=0, voxels_erased=0)
    room.check_export()
    room.check_votes(a, ids3, poses, P1)                                            # the map and the buffers go on


def test_empty_map(lom):
    g = lom.VoxelGrid(0.5, 6)
    a, poses = room_archive(lom, [300, 200], seed=79)
    ref = V.vote(np.zeros((0, 3), np.float32), 0.5, a.scans, [0, 1], poses, P1)
    assert ref["stats"]["rays_walked"] > 400 and ref["stats"]["cells_visited"] > 1000
    assert g.carveScans(a.dev, [0, 1], poses, P1) == ref["stats"]
    free, seen = g.scanVotes(a.dev, [0, 1], poses, P1)
    assert len(free) == 0 and len(seen) == 0 and g.size() == 0


# ---- 8: an armed cleanup scan ----------------------------------------------------------------------------------------------
def test_armed_scan_is_not_taken_across_the_votes(lom):
    """Arm, align, carveScans, radiusCleanup at the align's result: the scan behind the align is in flight (the control --
    the same sequence without the votes -- takes it) and the cleanup after the votes does not take it; the map equals the
    unarmed sequence's."""
    case = scenes.small_synth_case()
    p = V.params(0.3, 1.0, 30.0, 0.0, 1, 0)
    taken = lom.capi.COUNTER_CLEANUPS_BEHIND_ALIGN
    guess = ((0.05, -0.02, 0.0), scenes.angle_axis_q(0.01, (0, 0, 1)))
    radius = 6.0
    a = Archive(lom, [(case["scan"], np.ones_like(case["scan"]))])
    out = {}
    for what in ("control", "armed", "unarmed"):
        g = lom.VoxelGrid(0.5, 20)
        g.addCloud(case["map_xyz"], case["map_nrm"])
        g.radiusCleanup((0, 0, 0), 1e6)  # (sizes the cleanup's scratch: a scan behind an align does not allocate)
        if what != "unarmed":
            g.radiusCleanupAfterAlign(radius)
        pose = lom.CloudMatcher().align(g, case["scan"], lom.Pose3D(*guess))
        centre = np.asarray(pose.translation, np.float32)
        st = None
        if what != "control":
            st = g.carveScans(a.dev, [0], np.r_[pose.translation.astype(np.float64), pose.rotation.astype(np.float64)][None], p)
        before = g.debugCounter(taken)
        g.radiusCleanup(centre, radius)
        assert g.debugCounter(taken) - before == (1 if what == "control" else 0), what
        out[what] = (g.size(), g.getCloud(), st, centre.tobytes())
    (na, (xa, nrm_a), sa, ca), (nb, (xb, nrm_b), sb, cb) = out["armed"], out["unarmed"]
    assert ca == cb and na == nb and sa == sb and xa.tobytes() == xb.tobytes() and nrm_a.tobytes() == nrm_b.tobytes()
    assert sa["voxels_erased"] > 0 and na < out["control"][0]   # the votes' erasures are in the result


# ---- 9: determinism --------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(lom, oracle):
    got = []
    for _ in range(2):
        pair = room_pair(lom, oracle, seed=8)
        a, poses = room_archive(lom, [257] * 9, seed=80, ghosts=ghosts_of(pair))
        free, seen = pair.g.scanVotes(a.dev, np.arange(9), poses, P1)
        st = pair.g.carveScans(a.dev, np.arange(9), poses, V.params(0.3, 0.5, 8.0, 0.4, 2, 1))
        x, n = pair.g.getCloud()
        got.append((free.tobytes(), seen.tobytes(), tuple(sorted(st.items())), x.tobytes(), n.tobytes()))
    assert got[0] == got[1] and got[0][2] != ()


# ---- the mover scene -------------------------------------------------------------------------------------------------------
def test_mover_scene_equals_the_reference(lom):
    """The scene of tests/vote_scene.py assembled on the device (0.5 m voxels, 20 points each): votes and carve equal the
    reference's on the device's own export.  Only equality is asserted here; the scene's conditions are the reference's
    (tests/test_vote_host.py)."""
    s = S.scene(True)
    a = Archive(lom, s["scans"])
    g = lom.VoxelGrid(S.VOXEL, 20)
    g.assemble(a.dev, s["ids"], s["poses"])
    x, n = g.getCloud()
    ref = V.vote(x, S.VOXEL, a.scans, s["ids"], s["poses"], S.PARAMS)
    assert not ref["error"] and ref["stats"]["voxels_erased"] > 300
    free, seen = g.scanVotes(a.dev, s["ids"], s["poses"], S.PARAMS)
    assert np.array_equal(free, ref["free"]) and np.array_equal(seen, ref["seen"])
    assert g.carveScans(a.dev, s["ids"], s["poses"], S.PARAMS) == ref["stats"]
    x2, n2 = g.getCloud()
    assert x2.tobytes() == x[ref["point_keep"]].tobytes() and n2.tobytes() == n[ref["point_keep"]].tobytes()


# ---- 10: mirrors -----------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path, lom, oracle):
    """VoxelGrid::carveScans / scanVotes of the C++ mirror compile with plain g++ and leave what the Python calls leave."""
    exe = cpp_program.build_with_library(tmp_path, "test_vote.cpp")
    stdout = cpp_program.run(exe, timeout=120)
    size, erased = [int(v) for v in stdout.split()[-2:]]
    # the same map and scans here (tests/cpp/test_vote.cpp)
    c = np.arange(-4, 5)
    cells = np.stack([a.ravel() for a in np.meshgrid(c, c, c, indexing="ij")], 1).astype(np.float32)
    xyz = (cells * np.float32(0.5) + np.float32(0.125) * np.sign(cells)).astype(np.float32)
    pair = VPair(lom, oracle, 0.5, 4, xyz, np.zeros_like(xyz))
    pts = np.array([[2.1, 0.3 * k - 2.0, 0.2 * k - 1.0] for k in range(12)], np.float32)
    a = Archive(lom, [(pts, np.tile(np.float32([-1, 0, 0]), (12, 1)))])
    poses = np.array([[0.1, 0.1, 0.1, 1, 0, 0, 0], [0.1, 0.3, 0.1, 1, 0, 0, 0], [0.1, 0.1, 0.3, 1, 0, 0, 0]])
    ref = pair.check_carve(a, [0, 0, 0], poses, V.params(0.25, 0.5, 6.0, 0.3, 2, 1))
    assert (size, erased) == (pair.g.size(), ref["stats"]["voxels_erased"])
