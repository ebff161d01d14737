"""lom_archive_* and lom_map_assemble on the GPU against tests/assemble_ref.py.  The reference cloud is numpy f64
(quaternion to R, transform, cull, as the header states them); the reference MAP is the library's own, oracle-pinned insert:
a second VoxelGrid of the same voxel size and max_points and one addCloud of that cloud.  Everything is compared as bytes:
getCloud() points and normals, size(), pointCount(), the stats.  There is no tolerance anywhere in this file."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import assemble_ref as ref

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])
FAR = np.array([1234.56789, -987.654321, 12.3456789, 0.9, 0.1, -0.3, 0.2])  # unnormalised on purpose
SIZES = (0, 1, 63, 64, 65, 257, 1000)


@functools.lru_cache(maxsize=None)
def _scans(sizes, seed=0, spread=6.0):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        xyz = (rng.normal(size=(n, 3)) * spread).astype(np.float32)
        nrm = rng.normal(size=(n, 3)).astype(np.float32)
        out.append((xyz, nrm))
    return tuple(out)


def _poses(count, seed=1, t_scale=3.0):
    """generic rotations (unnormalised, w of either sign) with moderate translations"""
    rng = np.random.default_rng(seed)
    p = np.zeros((count, 7))
    p[:, :3] = rng.normal(size=(count, 3)) * t_scale
    p[:, 3:] = rng.normal(size=(count, 4)) * rng.uniform(0.5, 2.0, size=(count, 1))
    return p


def _archive(lom, scans, point_hint=0, scan_hint=0):
    a = lom.ScanArchive(point_hint, scan_hint)
    for k, (x, n) in enumerate(scans):
        assert a.add(x, n) == k
    return a


def _state(g):
    xyz, nrm = g.getCloud()
    return xyz.tobytes(), nrm.tobytes(), g.size(), g.pointCount()


def _check(lom, a, scans, ids, poses, voxel=0.5, cap=10, centre=None, radius=0.0, into=None):
    """assemble into a fresh map (or `into`) and compare with addCloud of the reference cloud; returns the state"""
    cx, cn = ref.concatenated(scans, ids, poses, centre, radius)
    g = into if into is not None else lom.VoxelGrid(voxel, cap)
    want = lom.VoxelGrid(voxel, cap)
    before = (0, 0)
    if into is not None:  # the copy: the same export re-added
        x0, n0 = into.getCloud()
        want.addCloud(x0, n0)
        assert _state(want) == _state(into)
        before = (into.size(), into.pointCount())
    want.addCloud(cx, cn)
    st = g.assemble(a, ids, poses, centre, radius)
    got = _state(g)
    assert got[2:] == _state(want)[2:]
    assert got == _state(want)
    assert st == dict(scans=len(ids), points_in=int(sum(len(scans[int(i)][0]) for i in ids)), points_kept=len(cx),
                      voxels_before=before[0], voxels_after=want.size(), points_stored_after=want.pointCount())
    return got, st


def test_scan_sizes_and_poses_four_kernel_insert(lom):
    scans = _scans(SIZES)
    a = _archive(lom, scans)
    assert len(a) == len(SIZES) and a.pointCount() == sum(SIZES) and [a.scanSize(k) for k in range(len(SIZES))] == list(SIZES)
    ids = np.arange(len(SIZES))
    poses = _poses(len(SIZES))
    poses[0], poses[2], poses[5] = FAR, IDENT, FAR  # an empty scan first; identity; the far f64 translation
    got, st = _check(lom, a, scans, ids, poses)
    assert st["points_in"] == sum(SIZES) < 65536 and st["voxels_after"] > 100
    # the f64 path carries weight: with that pose rounded to f32 first the reference cloud differs in at least one bit
    rounded = poses.copy()
    rounded[5] = FAR.astype(np.float32).astype(np.float64)
    x64, _ = ref.concatenated(scans, ids, poses)
    x32, _ = ref.concatenated(scans, ids, rounded)
    assert (x64.view(np.uint32) != x32.view(np.uint32)).any()
    # all identity: the archive's own bytes in call order
    _check(lom, a, scans, ids, np.tile(IDENT, (len(SIZES), 1)))
    # empty calls change nothing
    g = lom.VoxelGrid(0.5, 10)
    assert g.assemble(a, [], np.empty((0, 7)))["scans"] == 0 and g.size() == 0
    assert g.assemble(a, [0, 0], np.stack([FAR, IDENT]))["points_in"] == 0 and g.size() == 0
    assert g.assemble(a, [6], IDENT[None], centre=(500, 0, 0), radius=1.0)["points_kept"] == 0 and g.size() == 0


def test_bulk_insert_path(lom):
    scans = _scans((1000,) * 66, seed=2, spread=15.0)
    a = _archive(lom, scans, point_hint=66000, scan_hint=66)
    poses = _poses(66, seed=3, t_scale=10.0)
    got, st = _check(lom, a, scans, np.arange(66), poses)
    assert st["points_in"] == 66000 > 65536
    # ... and with a cull that leaves more than 65,536 of a larger call
    ids = np.concatenate([np.arange(66), np.arange(20)])
    poses2 = np.concatenate([poses, _poses(20, seed=4, t_scale=10.0)])
    got, st = _check(lom, a, scans, ids, poses2, centre=(1.0, -2.0, 0.5), radius=45.0)
    assert 65536 < st["points_kept"] < st["points_in"] == 86000


def test_order_is_the_priority(lom):
    scans = _scans((300, 257, 129, 64), seed=5, spread=1.0)  # overlapping: every voxel sees several scans
    a = _archive(lom, scans)
    ids = np.arange(4)
    poses = _poses(4, seed=6, t_scale=0.2)
    fwd, _ = _check(lom, a, scans, ids, poses, cap=2)
    rev, _ = _check(lom, a, scans, ids[::-1], poses[::-1], cap=2)
    assert fwd[:2] != rev[:2]


def test_repeated_id(lom):
    scans = _scans((257, 65), seed=7)
    a = _archive(lom, scans)
    poses = _poses(3, seed=8)
    _, st = _check(lom, a, scans, [0, 1, 0], poses)
    assert st["points_in"] == 257 + 65 + 257


def test_cull_boundary(lom):
    pts = np.array([[3, 4, 0], [3, 4, 1e-3], [0, 0, 5]], np.float32)
    nrm = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    a = _archive(lom, [(pts, nrm)])
    g = lom.VoxelGrid(0.5, 10)
    st = g.assemble(a, [0], IDENT[None], centre=(0, 0, 0), radius=5.0)
    xyz, n = g.getCloud()
    assert st["points_in"] == 3 and st["points_kept"] == 2
    assert xyz.tobytes() == pts[[0, 2]].tobytes() and n.tobytes() == nrm[[0, 2]].tobytes()
    _check(lom, a, [(pts, nrm)], [0], IDENT[None], centre=(0, 0, 0), radius=5.0)


def test_generic_cull(lom):
    # scan 1 sits 100 m away (culled whole); scan 0 is spread so that whole workgroups of 256 fall outside; scan 3 straddles
    rng = np.random.default_rng(9)
    s0 = (rng.normal(size=(1000, 3)) * 2).astype(np.float32)
    s0[256:768] += np.float32(60.0)  # workgroups 1 and 2 of scan 0
    far = (rng.normal(size=(300, 3)) * 2 + 100).astype(np.float32)
    mid = (rng.normal(size=(257, 3)) * 8).astype(np.float32)
    scans = [(s0, _scans((1000,), 10)[0][1]), (far, _scans((300,), 11)[0][1]), _scans((0,))[0], (mid, _scans((257,), 12)[0][1])]
    a = _archive(lom, scans)
    ids = [0, 1, 2, 3, 1]
    poses = np.tile(IDENT, (5, 1))
    poses[3] = [0.5, -0.25, 0.125, 0.7, -0.1, 0.2, 0.6]
    _, st = _check(lom, a, scans, ids, poses, centre=(0.5, 0.0, -0.5), radius=10.0)
    assert 0 < st["points_kept"] < st["points_in"] - 512 - 600
    _, st = _check(lom, a, scans, ids, poses, centre=(0.5, 0.0, -0.5), radius=1000.0)  # removes nothing at all
    assert st["points_kept"] == st["points_in"]
    _, st = _check(lom, a, scans, [1, 1], poses[:2], centre=(0, 0, 0), radius=10.0)  # whole scans, everything
    assert st["points_kept"] == 0 and st["voxels_after"] == 0


def test_atomicity_and_refusals(lom):
    import torch

    scans = list(_scans((257, 64, 300), seed=13))
    a = _archive(lom, scans)
    g = lom.VoxelGrid(0.5, 10)
    g.assemble(a, [0], IDENT[None])
    before = _state(g)
    poses = np.tile(IDENT, (3, 1))
    poses[2, 0] = 0.5 * float(1 << 20) - float(scans[2][0][:, 0].max()) + 1.0  # one point of the last scan at |x / voxel| >= 2^20
    x, _ = ref.concatenated(scans, [2], poses[2:])
    assert 1 <= int((np.abs(x[:, 0] / np.float32(0.5)) >= 2 ** 20).sum()) < 300
    for kw in (dict(), dict(centre=(0, 0, 0), radius=1e7)):
        with pytest.raises(lom.LomError) as e:
            g.assemble(a, [0, 1, 2], poses, **kw)
        assert e.value.code == lom.capi.ERR_RANGE
        assert _state(g) == before
    # a NaN planted through the device entry (the host entry refuses it)
    bad = scans[1][0].copy()
    bad[17, 1] = np.nan
    with pytest.raises(lom.LomError) as e:
        a.add(bad, scans[1][1])
    assert e.value.code == lom.capi.ERR_ARG and len(a) == 3 and a.pointCount() == 621
    dx, dn = torch.from_numpy(bad).to("cuda:0"), torch.from_numpy(scans[1][1]).to("cuda:0")
    torch.cuda.synchronize()
    assert a.addDevice(dx.data_ptr(), dn.data_ptr(), 64) == 3
    for kw in (dict(), dict(centre=(0, 0, 0), radius=1e7)):
        with pytest.raises(lom.LomError) as e:
            g.assemble(a, [1, 0, 3], np.tile(IDENT, (3, 1)), **kw)
        assert e.value.code == lom.capi.ERR_RANGE
        assert _state(g) == before
    # refusals before any launch: the map and the archive stay as they were
    L = lom.capi.lib()
    for ids, p in (([4], IDENT[None]), ([-1], IDENT[None]), ([0], np.array([[0, 0, 0, 0, 0, 0, 0.0]])),
                   ([0, 1], np.array([IDENT, [np.nan, 0, 0, 1, 0, 0, 0]])), ([0], np.array([[0, 0, 0, 1, np.inf, 0, 0]]))):
        with pytest.raises(lom.LomError) as e:
            g.assemble(a, ids, p)
        assert e.value.code == lom.capi.ERR_ARG
    with pytest.raises(lom.LomError) as e:
        g.assemble(a, [0], IDENT[None], centre=(0, np.nan, 0), radius=1.0)
    assert e.value.code == lom.capi.ERR_ARG
    ids64, p64 = np.zeros(1, np.int64), np.zeros(1, lom.capi.GRAPH_POSE)
    p64["q_wxyz"][0, 0] = 1.0
    assert L.lom_map_assemble(g.handle, a.handle, None, p64.ctypes.data, 1, None, None) == lom.capi.ERR_ARG
    assert L.lom_map_assemble(g.handle, a.handle, ids64.ctypes.data, None, 1, None, None) == lom.capi.ERR_ARG
    assert L.lom_map_assemble(g.handle, a.handle, ids64.ctypes.data, p64.ctypes.data, (1 << 24) + 1, None, None) == lom.capi.ERR_ARG
    ctx = lom.ScanContext(g)
    assert L.lom_map_assemble(ctx.handle, a.handle, ids64.ctypes.data, p64.ctypes.data, 1, None, None) == lom.capi.ERR_ARG
    assert L.lom_archive_scan_size(a.handle, 4) == lom.capi.ERR_ARG and L.lom_archive_get(a.handle, -1, None, None, 0) == lom.capi.ERR_ARG
    assert L.lom_archive_add(a.handle, scans[0][0].ctypes.data, None, 5, 12) == lom.capi.ERR_ARG
    assert L.lom_archive_add(a.handle, scans[0][0].ctypes.data, scans[0][1].ctypes.data, 5, 10) == lom.capi.ERR_ARG
    assert _state(g) == before and len(a) == 4
    # the map still works
    g2 = lom.VoxelGrid(0.5, 10)
    g2.assemble(a, [0], IDENT[None])
    g.assemble(a, [], np.empty((0, 7)))
    assert _state(g) == _state(g2)


def test_non_empty_target(lom):
    scans = _scans((1000, 257, 65), seed=14, spread=3.0)
    a = _archive(lom, scans)
    g = lom.VoxelGrid(0.5, 4)
    base = _scans((500,), seed=15, spread=3.0)[0]
    g.addCloud(*base)
    _check(lom, a, scans, [2, 0, 1], _poses(3, seed=16, t_scale=1.0), cap=4, into=g)
    _check(lom, a, scans, [1, 1], _poses(2, seed=17, t_scale=1.0), cap=4, into=g, centre=(0, 0, 0), radius=4.0)


def test_determinism_growth_and_round_trip(lom):
    scans = _scans(SIZES + (1000, 3000), seed=18)
    ids = np.array([8, 6, 5, 4, 3, 2, 1, 0, 7, 5])
    poses = _poses(len(ids), seed=19)
    grown = _archive(lom, scans, point_hint=1, scan_hint=1)  # grows through every add
    sized = _archive(lom, scans, point_hint=sum(len(x) for x, _ in scans), scan_hint=len(scans))
    runs = []
    for a in (grown, sized, grown):
        for kw in (dict(), dict(centre=(1, 2, 3), radius=9.0)):
            g = lom.VoxelGrid(0.5, 10)
            g.assemble(a, ids, poses, **kw)
            runs.append(_state(g))
    assert runs[0] == runs[2] == runs[4] and runs[1] == runs[3] == runs[5] and runs[0] != runs[1]
    for a in (grown, sized):
        for k, (x, n) in enumerate(scans):
            gx, gn = a.get(k)
            assert gx.tobytes() == x.tobytes() and gn.tobytes() == n.tobytes()
    # a strided host cloud (16-byte records) stores the same bytes
    rec = np.zeros((257, 4), np.float32)
    recn = np.zeros((257, 4), np.float32)
    rec[:, :3], recn[:, :3] = scans[5]
    k = lom.capi.lib().lom_archive_add(grown.handle, rec.ctypes.data, recn.ctypes.data, 257, 16)
    assert k == len(scans) and grown.get(k)[0].tobytes() == scans[5][0].tobytes() and grown.get(k)[1].tobytes() == scans[5][1].tobytes()
    grown.clear()
    assert len(grown) == 0 and grown.pointCount() == 0 and grown.add(*scans[3]) == 0
    assert grown.get(0)[0].tobytes() == scans[3][0].tobytes()


def test_scans_from_another_stream(lom):
    import torch

    scans = _scans((1000, 257, 64, 3000), seed=20)
    ids = np.array([3, 1, 0, 2, 1])
    poses = _poses(len(ids), seed=21)
    host = _archive(lom, scans)
    want = lom.VoxelGrid(0.5, 10)
    want.assemble(host, ids, poses)
    dev = lom.ScanArchive(1, 1)
    s = torch.cuda.Stream()
    keep = []
    for k, (x, n) in enumerate(scans):
        with torch.cuda.stream(s):
            if k == 1:  # 16-byte records
                tx = torch.zeros((len(x), 4), dtype=torch.float32, device="cuda:0")
                tn = torch.zeros((len(x), 4), dtype=torch.float32, device="cuda:0")
                tx[:, :3] = torch.from_numpy(x).to("cuda:0", non_blocking=True)
                tn[:, :3] = torch.from_numpy(n).to("cuda:0", non_blocking=True)
                stride = 16
            else:  # produced on the stream by arithmetic that keeps the bits
                tx = torch.from_numpy(x).to("cuda:0", non_blocking=True) * 1.0
                tn = torch.from_numpy(n).to("cuda:0", non_blocking=True) * 1.0
                stride = 12
            ev = torch.cuda.Event()
            ev.record(s)
        keep.append((tx, tn))
        assert dev.addDevice(tx.data_ptr(), tn.data_ptr(), len(x), stride, hip_event=C.c_void_p(ev.cuda_event)) == k
    for k, (x, n) in enumerate(scans):
        gx, gn = dev.get(k)
        assert gx.tobytes() == x.tobytes() and gn.tobytes() == n.tobytes()
    g = lom.VoxelGrid(0.5, 10)
    g.assemble(dev, ids, poses)
    assert _state(g) == _state(want)
    torch.cuda.synchronize()
