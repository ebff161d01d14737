"""Ray carving on the device against tests/carve_ref.py: crossing counts and hit flags per live voxel exactly equal,
and after a carve the size, the full export (points and normals, byte for byte) and every stats field exactly equal."""
import numpy as np
import pytest

from tests import carve_ref as R
from tests import cpp_program
from tests import scenes

pytestmark = pytest.mark.gpu

P1 = R.params(margin=0.25, min_range=0.5, max_range=6.0, min_crossings=1)


# ---- maps ---------------------------------------------------------------------------------------------------------------
def lattice_points(voxel, half):
    """one point in every cell of the block [-half, half]^3 of cell indices (a map without free space: every cell a
    walk visits is counted), normals from the index so that they are told apart"""
    c = np.arange(-half, half + 1)
    ix, iy, iz = [a.ravel() for a in np.meshgrid(c, c, c, indexing="ij")]
    idx = np.stack([ix, iy, iz], 1).astype(np.float64)
    lo, hi = R.cell_bounds(idx, float(np.float32(voxel)))
    xyz = (lo + (hi - lo) * 0.37).astype(np.float32)
    assert (R.map_index(xyz, voxel)[0] == idx).all()
    nrm = (idx / (half + 1)).astype(np.float32)
    return xyz, nrm


def room_points(seed=3, n_wall=4000, n_ghost=600):
    """walls of a 9 x 7 x 3.4 m room seen from inside, and ghosts: clutter in mid-air"""
    rng = np.random.default_rng(seed)
    h = np.array([4.5, 3.5, 1.7])
    face = rng.integers(0, 6, n_wall)
    wall = rng.uniform(-1, 1, (n_wall, 3)) * h
    wall[np.arange(n_wall), face // 2] = np.where(face % 2 == 0, -1.0, 1.0) * h[face // 2] + rng.normal(0, 0.01, n_wall)
    ghost = rng.uniform(-1, 1, (n_ghost, 3)) * (h - 0.8)
    xyz = np.concatenate([wall, ghost]).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    nrm = rng.normal(size=xyz.shape).astype(np.float32)
    return xyz, nrm


def room_rays(n, seed=5):
    """endpoints on the same walls (another sample), from an origin off-centre"""
    rng = np.random.default_rng(seed)
    h = np.array([4.5, 3.5, 1.7])
    face = rng.integers(0, 6, n)
    p = rng.uniform(-1, 1, (n, 3)) * h
    p[np.arange(n), face // 2] = np.where(face % 2 == 0, -1.0, 1.0) * h[face // 2] + rng.normal(0, 0.01, n)
    return np.array([0.3, -0.2, 0.1], np.float32), p.astype(np.float32)


class Pair:
    """a device map and the state the reference expects of it: the oracle's export, then whatever the carves leave"""

    def __init__(self, lom, O, voxel, K, xyz, nrm, hint=0, batches=1):
        self.lom, self.O, self.voxel, self.K = lom, O, voxel, K
        self.g = lom.VoxelGrid(voxel, K, capacity_hint=hint)
        og = O.VoxelGrid(voxel, K)
        for part_x, part_n in zip(np.array_split(xyz, batches), np.array_split(nrm, batches)):
            self.g.addCloud(part_x, part_n)
            og.addCloud(part_x, part_n)
        self.take(og)

    def take(self, og):
        self.xyz, self.nrm = og.getCloud()

    def oracle(self):
        return R.regrow(self.O, self.voxel, self.K, self.xyz, self.nrm)

    def check_export(self):
        keys, _ = R.voxels_of_export(self.xyz, self.voxel)
        assert self.g.size() == len(keys)
        gx, gn = self.g.getCloud()
        assert gx.tobytes() == self.xyz.tobytes() and gn.tobytes() == self.nrm.tobytes()

    def check_counts(self, origin, pts, p):
        ref = R.carve(self.xyz, self.voxel, origin, pts, p)
        assert not ref["error"]
        cross, hit = self.g.carveCounts(origin, pts, p)
        assert np.array_equal(cross, ref["cross"]), np.flatnonzero(cross != ref["cross"])[:10]
        assert np.array_equal(hit, ref["hit"])
        return ref

    def check_carve(self, origin, pts, p, **how):
        ref = R.carve(self.xyz, self.voxel, origin, pts, p)
        assert not ref["error"]
        st = self.g.carveRays(origin, pts, p, **how)
        print("carve", st)
        assert st == ref["stats"]
        self.xyz, self.nrm = self.xyz[ref["point_keep"]], self.nrm[ref["point_keep"]]
        self.check_export()
        return ref


@pytest.fixture(scope="module")
def lattice(lom, oracle):
    xyz, nrm = lattice_points(0.5, 6)
    return Pair(lom, oracle, 0.5, 4, xyz, nrm)


@pytest.fixture(scope="module")
def room(lom, oracle):
    xyz, nrm = room_points()
    return Pair(lom, oracle, 0.2, 6, xyz, nrm)


# ---- the walk, cell by cell (counts only: nothing is erased, the maps are shared) --------------------------------------
PLANE_RULE = [  # (origin, endpoints): voxel 0.5
    ([0.2, 0.1, 0.15], [[2.3, 0.1, 0.15], [-2.3, 0.1, 0.15], [0.2, 2.2, 0.15], [0.2, -2.2, 0.15], [0.2, 0.1, 2.4],
                        [0.2, 0.1, -2.4], [-1.9, -2.1, -1.3], [1.7, -1.2, 2.3]]),                  # origin in cell 0
    ([-0.7, -0.6, -0.8], [[2.3, -0.6, -0.8], [-0.7, 2.2, -0.8], [-0.7, -0.6, 2.4], [1.9, 2.1, 1.3], [-2.4, -2.2, -2.9],
                          [1.1, -2.0, 0.4]]),                                                       # origin in cell -1
    ([0.5, -0.5, 1.0], [[2.3, 1.9, -1.4], [-2.3, -1.9, 2.6], [-2.0, 0.3, 0.2], [0.5, -0.5, -2.0], [2.5, -0.5, 1.0],
                        [-1.5, -2.5, 3.0]]),                                                        # origin on planes
]


@pytest.mark.parametrize("case", range(len(PLANE_RULE)))
def test_plane_rule(lattice, case):
    origin, pts = PLANE_RULE[case]
    ref = lattice.check_counts(origin, pts, R.params(0.0, 0.1, 10.0, 1))
    assert ref["stats"]["rays_walked"] == len(pts) and ref["cross"].max() >= 2


def test_axis_parallel_rays(lattice):
    origin = [0.25, 0.75, -0.6]
    pts = [[2.6, 0.75, -0.6], [-2.6, 0.75, -0.6], [0.25, 2.9, -0.6], [0.25, 0.75, 2.2], [2.1, 2.3, -0.6], [0.25, -2.2, 1.9]]
    lattice.check_counts(origin, pts, R.params(0.1, 0.1, 10.0, 1))
    # rays that lie in a plane (y = 0.5 is one), along x and along the diagonal of that plane
    lattice.check_counts([0.3, 0.5, 0.2], [[2.7, 0.5, 0.2], [-2.7, 0.5, 0.2], [2.3, 0.5, 2.2]], R.params(0.1, 0.1, 10.0, 1))


def test_exact_ties(lattice):
    """lattice diagonals: two- and three-way ties in t_a, every one broken x before y before z"""
    origin = [0.25, 0.25, 0.25]
    pts = [[2.25, 2.25, 2.25], [-2.75, -2.75, -2.75], [2.25, 2.25, 0.25], [2.25, 0.25, 2.25], [0.25, -2.75, -2.75],
           [2.25, -1.75, 2.25], [-2.75, 2.25, 0.25]]
    p = R.params(0.0, 0.1, 10.0, 1)
    ref = lattice.check_counts(origin, pts, p)
    w = R.walk(origin, pts[:1], 0.5, p)
    assert w["cell"][:4].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]]  # the three intermediate cells in order
    assert ref["stats"]["cells_visited"] > 3 * len(pts)


def test_length_rules(lattice):
    origin = [0.25, 0.25, 0.25]
    p = R.params(margin=0.25, min_range=0.5, max_range=2.5, min_crossings=1)
    pts = [[0.25, 0.25, 0.25],   # L == 0
           [0.55, 0.25, 0.25],   # L < min_range
           [2.25, 0.25, 0.25],   # t_end exactly on the plane x = 2.0: the cell behind it is entered
           [0.25, 2.9, 0.25],    # L > max_range: walked to 2.5 - 0.25
           [-2.6, 1.4, -0.8]]
    ref = lattice.check_counts(origin, pts, p)
    assert ref["stats"]["rays_walked"] == 3 and ref["stats"]["rays_skipped"] == 2
    w = R.walk(origin, pts[2:3], 0.5, p)
    assert w["cell"][-1].tolist() == [4, 0, 0]
    # L in (min_range, margin]: t_end <= 0, not walked
    ref = lattice.check_counts(origin, [[1.0, 0.25, 0.25], [0.25, 1.25, 0.25]], R.params(1.0, 0.5, 2.5, 1))
    assert ref["stats"]["rays_walked"] == 0 and not ref["cross"].any() and ref["hit"].sum() == 2


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_ray_counts_and_order(room, n):
    origin, pts = room_rays(n, seed=100 + n)
    p = R.params(0.3, 0.5, 5.0, 2)
    ref = room.check_counts(origin, pts, p)
    if n > 1:
        again = room.g.carveCounts(origin, pts[np.random.default_rng(1).permutation(n)], p)
        assert np.array_equal(again[0], ref["cross"]) and np.array_equal(again[1], ref["hit"])
    if n == 4097:
        assert ref["cross"].max() > 50 and ref["hit"].sum() > 500 and ref["erase"].sum() > 100


# ---- the decision and the erase ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_crossings", [1, 3])
def test_thresholds(lom, oracle, min_crossings):
    xyz, nrm = room_points(seed=8)
    pair = Pair(lom, oracle, 0.2, 6, xyz, nrm)
    origin, pts = room_rays(4000, seed=9)
    d = np.linalg.norm(xyz - origin, axis=1)
    near = xyz[(d > 0.5) & (d < 0.9)][:5]                             # ghosts near the origin, hit by rays of their own
    assert len(near) == 5
    ref = pair.check_carve(origin, np.concatenate([pts, near]), R.params(0.3, 0.4, 8.0, min_crossings))
    assert ref["stats"]["voxels_erased"] > 20
    assert ((ref["cross"] >= 5) & (ref["hit"] > 0)).any()           # a hit voxel that many other rays cross is kept
    assert ref["stats"]["voxels_protected"] > 0
    if min_crossings == 3:
        assert ((ref["cross"] > 0) & (ref["cross"] < 3) & (ref["hit"] == 0)).any()  # crossed, but not often enough


def test_in_place_erase_holes_device_entry_and_reinsert(lom, oracle):
    xyz, nrm = room_points(seed=12)
    pair = Pair(lom, oracle, 0.2, 6, xyz, nrm)
    nv = pair.g.size()
    origin, pts = room_rays(400, seed=13)
    ref = pair.check_carve(origin, pts, R.params(0.3, 0.5, 8.0, 2))
    erased = ref["stats"]["voxels_erased"]
    assert 0 < erased * 4 <= nv
    assert pair.g.debugCounter(lom.capi.COUNTER_EMPTY_SLABS) == erased   # in place: the slabs stay, empty
    # a carve over a map with those holes; the host and the device entry points agree
    import ctypes as C
    origin2, pts2 = room_rays(500, seed=14)
    L, ws, d = lom.capi.lib(), lom.VoxelGrid(0.5, 1), C.c_void_p()  # the rays in HBM: another handle's staging buffer
    lom.capi.check(L.lom_upload_points(ws.handle, pts2.ctypes.data, None, len(pts2), 12, C.byref(d), None), ws.handle)
    lom.capi.check(L.lom_map_status(ws.handle), ws.handle)            # (waits for that handle's copy)
    pair.check_carve(origin2, pts2, R.params(0.3, 0.5, 8.0, 1), device_ptr=d, n=len(pts2))
    # re-insert: a point into a carved voxel and one elsewhere; the carved voxel comes back at the end of the creation order
    gone = xyz[~np.isin(R.pack(R.map_index(xyz, 0.2)[0]), R.voxels_of_export(pair.xyz, 0.2)[0])]
    assert len(gone)
    new_x = np.concatenate([gone[:3], pair.xyz[:2]]).astype(np.float32)
    new_n = np.ones_like(new_x)
    og = pair.oracle()
    og.addCloud(new_x, new_n)
    pair.g.addCloud(new_x, new_n)
    pair.take(og)
    pair.check_export()
    assert R.pack(R.map_index(pair.xyz[-1:], 0.2)[0])[0] in set(R.pack(R.map_index(gone[:3], 0.2)[0]).tolist())


def test_compaction(lom, oracle):
    """the lattice has no free space: every crossed voxel without a hit goes, far more than a quarter"""
    xyz, nrm = lattice_points(0.5, 5)
    pair = Pair(lom, oracle, 0.5, 4, xyz, nrm)
    nv = pair.g.size()
    rng = np.random.default_rng(21)
    pts = rng.uniform(-2.7, 2.7, (1500, 3))
    pts[np.arange(1500), rng.integers(0, 3, 1500)] = rng.choice([-2.7, 2.7], 1500)  # endpoints in the outermost cells only
    pts = pts.astype(np.float32)
    ref = pair.check_carve([0.1, 0.2, -0.1], pts, R.params(0.3, 0.5, 6.0, 2))
    assert ref["stats"]["voxels_erased"] * 4 > nv
    assert pair.g.debugCounter(lom.capi.COUNTER_EMPTY_SLABS) == 0
    pair.check_counts([0.1, 0.2, -0.1], pts[:100], P1)  # the rebuilt table


def test_dense_switch(lom, oracle, monkeypatch):
    monkeypatch.setenv("LOM_DENSE_CLEANUP", "1")
    xyz, nrm = room_points(seed=12)
    pair = Pair(lom, oracle, 0.2, 6, xyz, nrm)
    origin, pts = room_rays(400, seed=13)
    ref = pair.check_carve(origin, pts, R.params(0.3, 0.5, 8.0, 2))
    assert 0 < ref["stats"]["voxels_erased"] * 4 <= len(ref["cross"])
    assert pair.g.debugCounter(lom.capi.COUNTER_EMPTY_SLABS) == 0


def test_holes_from_a_radius_cleanup(lom, oracle):
    xyz, nrm = room_points(seed=30)
    pair = Pair(lom, oracle, 0.2, 6, xyz, nrm)
    og = pair.oracle()
    centre = [1.5, 0.0, 0.0]
    og.radiusCleanup(centre, 6.2)   # an eighth of the voxels: erased in place
    pair.g.radiusCleanup(centre, 6.2)
    assert pair.g.debugCounter(lom.capi.COUNTER_EMPTY_SLABS) > 0
    pair.take(og)
    pair.check_export()
    origin, pts = room_rays(1500, seed=31)
    pair.check_counts(origin, pts, R.params(0.3, 0.5, 8.0, 2))
    pair.check_carve(origin, pts, R.params(0.3, 0.5, 8.0, 2))


def _hash(key, bits):
    """lom_internal.hpp's hash_key: the top `bits` bits of key * 2^64 / phi"""
    return ((int(key) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> (64 - bits)


def test_table_wrap(lom, oracle):
    """The smallest table (1,024 slots for a small capacity hint; inserts of at most 100 points into fewer than 400 voxels
    never grow it) with 60 voxels whose keys hash into its last six slots: their chains wrap around the table's end."""
    c = np.arange(-12, 13)
    cells = np.stack([a.ravel() for a in np.meshgrid(c, c, c, indexing="ij")], 1)
    h = np.array([_hash(k, 10) for k in R.pack(cells)])
    tail = cells[h >= 1018]
    assert len(tail) >= 60
    rng = np.random.default_rng(40)
    rest = cells[rng.permutation(len(cells))[:300]]
    pick = np.unique(np.concatenate([tail[:60], rest]), axis=0)
    pick = pick[rng.permutation(len(pick))]
    lo, hi = R.cell_bounds(pick.astype(np.float64), 0.5)
    xyz = (lo + (hi - lo) * 0.5).astype(np.float32)
    pair = Pair(lom, oracle, 0.5, 4, xyz, np.ones_like(xyz), hint=1, batches=4)
    pts = rng.uniform(-6.2, 6.2, (600, 3)).astype(np.float32)
    origin = [0.2, -0.3, 0.1]
    lo, hi = R.cell_bounds(tail[:60].astype(np.float64), 0.5)
    pts = np.concatenate([pts, (1.3 * (lo + hi) / 2).astype(np.float32)])  # and a ray through every one of the sixty
    ref = pair.check_counts(origin, np.concatenate([pts, xyz[:50]]), R.params(0.1, 0.5, 9.0, 1))
    tail_keys = set(R.pack(tail[:60]).tolist())
    keys, _ = R.voxels_of_export(pair.xyz, 0.5)
    crossed_tail = [k in tail_keys for k in keys[ref["cross"] > 0].tolist()]
    assert sum(crossed_tail) >= 10  # the wrapped chains were walked
    pair.check_carve(origin, np.concatenate([pts, xyz[:50]]), R.params(0.1, 0.5, 9.0, 1))


def test_armed_scan_is_not_taken_across_a_carve(lom, oracle):
    """Arm, align, carve, radiusCleanup at the align's result: the scan behind the align is in flight (the control -- the
    same sequence without the carve -- takes it) and the cleanup after a carve does not take it; the map equals the
    unarmed sequence's."""
    case = scenes.small_synth_case()
    p = R.params(0.3, 1.0, 30.0, 1)
    taken = lom.capi.COUNTER_CLEANUPS_BEHIND_ALIGN
    guess = ((0.05, -0.02, 0.0), scenes.angle_axis_q(0.01, (0, 0, 1)))  # five outer iterations: the scan finds the align finished
    radius = 6.0
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
            st = g.carveRays(centre, lom.transform_points(pose, case["scan"]), p)
        before = g.debugCounter(taken)
        g.radiusCleanup(centre, radius)
        assert g.debugCounter(taken) - before == (1 if what == "control" else 0), what
        out[what] = (g.size(), g.getCloud(), st, centre.tobytes())
    (na, (xa, nrm_a), sa, ca), (nb, (xb, nrm_b), sb, cb) = out["armed"], out["unarmed"]
    assert ca == cb and na == nb and sa == sb and xa.tobytes() == xb.tobytes() and nrm_a.tobytes() == nrm_b.tobytes()
    full = lom.VoxelGrid(0.5, 20)
    full.addCloud(case["map_xyz"], case["map_nrm"])
    assert sa["voxels_erased"] > 0 and na < full.size() - sa["voxels_erased"]  # both the carve and the cleanup erased
    assert na < out["control"][0]                                             # ... and the carve's erasures are in the result


@pytest.mark.parametrize("bad", [[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [0.5 * 2.0 ** 20, 1.0, 1.0], [1.0, 1.0, -0.5 * 2.0 ** 20]])
def test_range_errors_leave_the_map_alone(room, bad):
    lom = room.lom
    origin, pts = room_rays(200, seed=50)
    pts = pts.copy()
    pts[137] = bad
    for call in (lambda: room.g.carveRays(origin, pts, P1), lambda: room.g.carveCounts(origin, pts, P1),
                 lambda: room.g.carveRays(bad, pts[:100], P1)):
        with pytest.raises(lom.LomError) as e:
            call()
        assert e.value.code == lom.capi.ERR_RANGE
    assert R.carve(room.xyz, 0.2, origin, pts, P1)["error"]
    room.check_export()
    ok = room.g.carveRays(origin, np.zeros((0, 3), np.float32), P1)  # n == 0: nothing happens
    assert ok["rays_walked"] == 0 and ok["voxels_erased"] == 0
    room.check_export()


def test_empty_map(lom, oracle):
    """an empty map is a map like any other: the stats of the definition, the range verdict, nothing crossed"""
    g = lom.VoxelGrid(0.2, 6)
    origin, pts = room_rays(300, seed=60)
    ref = R.carve(np.zeros((0, 3), np.float32), 0.2, origin, pts, P1)
    assert ref["stats"]["rays_walked"] == 300 and ref["stats"]["cells_visited"] > 300 and ref["stats"]["voxels_crossed"] == 0
    assert g.carveRays(origin, pts, P1) == ref["stats"]
    cross, hit = g.carveCounts(origin, pts, P1)
    assert len(cross) == 0 and len(hit) == 0 and g.size() == 0
    bad = pts.copy()
    bad[7, 1] = np.nan
    for call in (lambda: g.carveRays(origin, bad, P1), lambda: g.carveCounts(origin, bad, P1),
                 lambda: g.carveRays([np.inf, 0.0, 0.0], pts, P1)):
        with pytest.raises(lom.LomError) as e:
            call()
        assert e.value.code == lom.capi.ERR_RANGE
    g.addCloud(pts[:50], np.ones_like(pts[:50]))  # the handle goes on
    assert g.size() > 0


def test_scan_context_is_refused(lom, room):
    import ctypes as C
    L = lom.capi.lib()
    ctx = C.c_void_p()
    assert L.lom_scan_create(room.g.handle, C.byref(ctx)) == 0
    try:
        origin, pts = room_rays(10)
        p = lom.carveParams(P1)
        assert L.lom_map_carve_rays(ctx, lom.capi.f3(origin), pts.ctypes.data, 10, 12, C.byref(p), None) == lom.capi.ERR_ARG
    finally:
        L.lom_scan_destroy(ctx)


def test_cpp_mirror(tmp_path, lom, oracle):
    """VoxelGrid::carveRays of the C++ mirror compiles with plain g++ and leaves the size the Python call leaves."""
    exe = cpp_program.build_with_library(tmp_path, "test_carve.cpp")
    size, erased = [int(v) for v in cpp_program.run(exe, timeout=120).split()[-2:]]
    # the same map and rays here (tests/cpp/test_carve.cpp)
    c = np.arange(-4, 5)
    cells = np.stack([a.ravel() for a in np.meshgrid(c, c, c, indexing="ij")], 1).astype(np.float32)
    xyz = (cells * np.float32(0.5) + np.float32(0.125) * np.sign(cells)).astype(np.float32)
    pair = Pair(lom, oracle, 0.5, 4, xyz, np.zeros_like(xyz))
    pts = np.array([[2.1, 0.3 * k - 2.0, 0.2 * k - 1.0] for k in range(12)], np.float32)
    ref = pair.check_carve([0.1, 0.1, 0.1], pts, R.params(0.25, 0.5, 6.0, 1))
    assert (size, erased) == (pair.g.size(), ref["stats"]["voxels_erased"])
