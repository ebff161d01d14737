"""Seeded walks over the map's public calls (test infrastructure of test_map_walks_host.py / test_map_walks_gpu.py).

walk(seed) draws about 30 calls with their arguments; play() runs them on the oracle's VoxelGrid and -- when given --
on a device VoxelGrid beside it, comparing as it goes.  The arguments never depend on device output, with one
exception: the centre of the cleanup that follows an align is the align's result (lidar_odometry.cpp:65-67), the
device's where there is a device, handed to both sides.

The cloud is the 6000 points of scenes.small_synth_case()'s map nearest the origin (a disc of about 15 m: as dense as the
map itself, so the scan aligns against it as it does against the whole map); voxel size 0.5; the cap drawn from {1, 3, 20}.
"""
import ctypes as C

import numpy as np

from tests import scenes

VOXEL = 0.5
CLOUD_POINTS = 6000
SEEDS = (4, 6, 11, 22, 28, 46)      # fixed (caps 20, 3, 1, 20, 3, 1): tests/test_map_walks_host.py holds each to survey()'s conditions
DENSE_SEEDS = SEEDS[:2]             # these also run with LOM_DENSE_CLEANUP=1
GUESS = ((0.05, -0.02, 0.0), scenes.angle_axis_q(0.01, (0, 0, 1)))
CARVE = dict(margin=0.25, min_range=0.5, max_range=6.0, min_crossings=1)
MUTATING = ("add", "add_nowait", "cleanup", "align_cleanup", "set_cap", "clear")
# the calls of test_map_call_order_gpu.py's table that a walk puts between an align and its cleanup
READERS = ("getCloud", "getSparseCloudWithoutNormals", "pointCount", "size", "findMatchingPairs", "quality", "carveCounts",
           "map_status")

_case = {}


def case():
    """(cloud xyz, cloud normals, scan, search queries) -- computed once, never written to"""
    if not _case:
        sm = scenes.small_synth_case()
        near = np.sort(np.argsort(np.linalg.norm(sm["map_xyz"].astype(np.float64), axis=1), kind="stable")[:CLOUD_POINTS])
        xyz, nrm = np.ascontiguousarray(sm["map_xyz"][near]), np.ascontiguousarray(sm["map_nrm"][near])
        rng = np.random.default_rng(11)
        queries = np.ascontiguousarray(xyz[np.sort(rng.choice(len(xyz), 1500, replace=False))] + np.float32(0.02))
        for a in (xyz, nrm, queries):
            a.setflags(write=False)
        _case.update(xyz=xyz, nrm=nrm, scan=sm["scan"], queries=queries,
                     reach=float(np.linalg.norm(xyz.astype(np.float64), axis=1).max()))
    return _case


def walk(seed):
    """dict(cap, steps): steps = [(kind, args...)], kinds as in play()"""
    c = case()
    rng = np.random.default_rng(1000 + seed)
    n_cloud, reach = len(c["xyz"]), c["reach"]
    cap = int(rng.choice([1, 3, 20]))

    def selection():
        return np.sort(rng.choice(n_cloud, int(rng.integers(500, 3001)), replace=False))

    def centre():
        return tuple(float(v) for v in np.float32([rng.uniform(-4, 4), rng.uniform(-4, 4), 0.0]))

    def radius():
        # from a ball that erases most of the disc to one that only trims its rim
        return float(np.float32(rng.uniform(5.0, reach + 1.0)))

    # the map is built by the first inserts, and a cleanup that erases nothing sizes the cleanup's scratch (a scan behind
    # an align does not allocate)
    steps = [("add", selection()), ("add", selection()), ("add", selection()), ("cleanup", (0.0, 0.0, 0.0), 1e6)]
    kinds = ["add", "add_nowait", "cleanup", "align_cleanup", "align_reader_cleanup", "set_cap", "export", "point_count",
             "pairs", "clear"]
    weights = np.array([5, 2, 4, 3, 3, 3, 2, 1, 1, 1], np.float64)
    cleared = False
    while len(steps) < 30:
        kind = str(rng.choice(kinds, p=weights / weights.sum()))
        if kind in ("add", "add_nowait"):
            steps.append((kind, selection()))
        elif kind == "cleanup":
            steps.append(("cleanup", centre(), radius()))
        elif kind == "align_cleanup":
            steps.append(("align_cleanup", radius(), None))
        elif kind == "align_reader_cleanup":
            steps.append(("align_cleanup", radius(), str(rng.choice(READERS))))
        elif kind == "set_cap":
            steps.append(("set_cap", int(rng.choice([1, 2, 3, 5, 20, 30]))))
        elif kind == "export":
            steps.append(("export", int(rng.integers(0, 3))))
        elif kind == "point_count":
            steps.append(("point_count",))
        elif kind == "pairs":
            steps.append(("pairs",))
        elif not cleared:  # setVoxelSize clears: once per walk, and the map is built again
            cleared = True
            steps += [("clear",), ("add", selection()), ("add", selection())]
    return dict(cap=cap, steps=steps)


def keys_of(xyz):
    """voxel key per point: the truncating index of voxel_grid.h, packed"""
    i = (np.asarray(xyz, np.float32) / np.float32(VOXEL)).astype(np.int64) + (1 << 20)
    return (i[:, 0] << 42) | (i[:, 1] << 21) | i[:, 2]


def _reader(name, g, lom, c):
    if name == "getCloud":
        g.getCloud()
    elif name == "getSparseCloudWithoutNormals":
        g.getSparseCloudWithoutNormals()
    elif name == "pointCount":
        g.pointCount()
    elif name == "size":
        g.size()
    elif name == "findMatchingPairs":
        g.findMatchingPairs(c["queries"], lom.Pose3D(), 0.3)
    elif name == "quality":
        g.quality(c["scan"], lom.Pose3D(*GUESS))
    elif name == "carveCounts":
        g.carveCounts((0.0, 0.0, 0.0), c["scan"][:64], CARVE)
    elif name == "map_status":
        assert lom.capi.lib().lom_map_status(g.handle) == 0
    else:
        raise ValueError(name)


def play(w, O, lom=None, after=None):
    """Run the walk on an oracle grid and, with `lom`, on a device grid beside it.  after(i, step, g, og, info) is called
    after every step; info: what the step found (sizes around a cleanup, the device's counters are the caller's to
    read).  Exports, point counts and searches are compared where both sides exist.  Returns (g, og)."""
    c = case()
    xyz, nrm = c["xyz"], c["nrm"]
    og = O.VoxelGrid(VOXEL, w["cap"])
    g = lom.VoxelGrid(VOXEL, w["cap"]) if lom else None
    om = O.CloudMatcher()
    m = lom.CloudMatcher() if lom else None
    ws = lom.VoxelGrid(VOXEL, 1) if lom else None  # (its staging buffer holds the no-wait insert's input)
    for i, step in enumerate(w["steps"]):
        kind, info = step[0], {}
        if kind == "add":
            sel = step[1]
            og.addCloud(xyz[sel], nrm[sel])
            if g:
                g.addCloud(xyz[sel], nrm[sel])
        elif kind == "add_nowait":
            sel = step[1]
            og.addCloud(xyz[sel], nrm[sel])
            if g:
                # the input in HBM: another handle's staging buffer, valid until that handle's next upload
                L, dx, dn = lom.capi.lib(), C.c_void_p(), C.c_void_p()
                px, pn = np.ascontiguousarray(xyz[sel]), np.ascontiguousarray(nrm[sel])
                lom.capi.check(L.lom_upload_points(ws.handle, px.ctypes.data, pn.ctypes.data, len(sel), 12, C.byref(dx), C.byref(dn)),
                               ws.handle)
                lom.capi.check(L.lom_map_status(ws.handle), ws.handle)   # (waits for that handle's copy)
                lom.capi.check(L.lom_map_add_points_device_nowait(g.handle, dx, dn, len(sel), 12), g.handle)
                assert L.lom_map_status(g.handle) == 0   # the verdict, later (the input stays valid until here)
        elif kind == "cleanup":
            info["before"] = og.size()
            og.radiusCleanup(step[1], step[2])
            if g:
                g.radiusCleanup(step[1], step[2])
        elif kind == "align_cleanup":
            r, reader = step[1], step[2]
            info["before"] = og.size()
            op = om.align(og, c["scan"], O.Pose3D(*GUESS))
            centre = np.asarray(op.translation, np.float32)
            if g:
                g.radiusCleanupAfterAlign(r)
                p = m.align(g, c["scan"], lom.Pose3D(*GUESS))
                assert m.stats["outer_iterations"] == om.stats["outer_iterations"], (i, step)
                centre = np.asarray(p.translation, np.float32)   # the device's result, handed to both sides
                if reader:
                    _reader(reader, g, lom, c)
                g.radiusCleanup(centre, r)
            og.radiusCleanup(centre, r)
        elif kind == "set_cap":
            og.setMaxPoints(step[1])
            if g:
                g.setMaxPoints(step[1])
        elif kind == "export":
            fn = ("getCloudWithoutNormals", "getSparseCloudWithoutNormals", "getCloud")[step[1]]
            ref = getattr(og, fn)()
            if g:
                got = getattr(g, fn)()
                assert np.asarray(got).tobytes() == np.asarray(ref).tobytes(), (i, step)
        elif kind == "point_count":
            assert g is None or g.pointCount() == og.pointCount(), (i, step)
        elif kind == "pairs":
            oc = og.findMatchingPairs(c["queries"], O.Pose3D(), 0.3)
            if g:
                assert np.array_equal(g.findMatchingPairs(c["queries"], lom.Pose3D(), 0.3)["index"], oc["index"]), (i, step)
        elif kind == "clear":
            og.setVoxelSize(VOXEL)
            if g:
                g.setVoxelSize(VOXEL)
        else:
            raise ValueError(kind)
        if after:
            after(i, step, g, og, info)
    return g, og


def survey(w, O):
    """The walk through the oracle alone: what makes it worth running.  dict(erasing: fraction of the voxels it met that
    each cleanup erased, in walk order, zeros left out; small_then_big: a cleanup erasing fewer than a quarter is followed
    by one erasing more than a quarter (or by the clear) -- empty slabs pile up, then go; recreated: inserts that created
    voxels a cleanup had erased; cap_lowered: setMaxPoints calls below what some voxel held; final_size)."""
    out = dict(erasing=[], small_then_big=False, recreated=0, cap_lowered=0, final_size=0)
    state = dict(erased=set(), live=set(), small_seen=False)

    def live_keys(og):
        return set(keys_of(og.getSparseCloudWithoutNormals()).tolist())

    def after(i, step, g, og, info):
        kind = step[0]
        if kind in ("cleanup", "align_cleanup"):
            now = live_keys(og)
            gone = state["live"] - now
            state["erased"] |= gone
            if gone:
                frac = len(gone) / info["before"]
                out["erasing"].append(frac)
                if frac < 0.25:
                    state["small_seen"] = True
                elif frac > 0.25 and state["small_seen"]:
                    out["small_then_big"] = True
            state["live"] = now
        elif kind in ("add", "add_nowait"):
            now = live_keys(og)
            back = (now - state["live"]) & state["erased"]
            if back:
                out["recreated"] += 1
                state["erased"] -= back
            state["live"] = now
        elif kind == "clear":
            if state["small_seen"]:
                out["small_then_big"] = True
            state["live"], state["erased"] = set(), set()
        out["final_size"] = og.size()

    # (the cap against what the voxels hold is looked at BEFORE the call: a wrapper around the steps)
    held = dict(max=0)

    def watch(i, step, g, og, info):
        after(i, step, g, og, info)
        nxt = w["steps"][i + 1] if i + 1 < len(w["steps"]) else None
        if nxt and nxt[0] == "set_cap" and og.size():
            _, counts = np.unique(keys_of(og.getCloudWithoutNormals()), return_counts=True)
            if nxt[1] < counts.max():
                out["cap_lowered"] += 1

    play(w, O, None, watch)
    return out
