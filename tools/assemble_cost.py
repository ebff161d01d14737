#!/usr/bin/env python3
"""What the map assembly costs against the same work done by the calls that existed before it: one JSON line.
Synthetic scans (synth.make_sequence_frame: classify, range filter, down-sampling at the update voxel size; about 8k
points each, repeated round robin to K), K in --scans, into an empty map of voxel 0.2 / 20 points per voxel, wall clock
around the calls (every variant ends with the map settled: size() is read).
    assemble_ms        one lom_map_assemble of the K scans at K f64 poses
    assemble_cull_ms   the same with the pipeline's cull (radius 80 m around the last pose)
    per_scan_ms        the yardstick: per scan lom_transform_points_device with the pose rounded to f32, then
                       lom_map_add_points_device, from device-resident copies of the same scans (not the same bytes as the
                       assembly: f32 poses and K inserts instead of one, so a voxel's survivors are the same but rounded
                       differently)
in --blocks alternating blocks, medians and ranges of the block values (one call per block and variant for K >= 64,
--calls for smaller K).
    python tools/assemble_cost.py [--scans 8,64,512] [--blocks 5] [--calls 5] > profiles/assemble_cost.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", default="8,64,512")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic frames behind the K scans")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi, synth

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    prm = lom.LidarOdometry().params
    ws = lom.VoxelGrid(0.5, 1)
    clouds = []
    for k in range(args.distinct):
        pxyz, pnrm, _, _ = lom.classify(lom.pointTimeNormalize(synth.make_sequence_frame(k * 10)))
        fx, fn = lom.rangeFilter(pxyz, pnrm, prm.lidar_min_range, prm.lidar_max_range)
        clouds.append(ws.downsample(fx, fn, prm.keyframe_update_voxel_size))
    dev = [(torch.from_numpy(x).cuda(), torch.from_numpy(n).cuda()) for x, n in clouds]
    torch.cuda.synchronize()
    out = {"device": torch.cuda.get_device_name(0), "points_per_scan": [len(x) for x, _ in clouds], "voxel": 0.2,
           "max_points": 20, "note": "ms per K scans, wall clock, map settled at the end", "K": {}}
    for K in [int(s) for s in args.scans.split(",")]:
        arch = lom.ScanArchive(sum(len(clouds[k % args.distinct][0]) for k in range(K)), K)
        for k in range(K):
            arch.add(*clouds[k % args.distinct])
        # a slow drive along x with a small yaw, as the sequence's
        poses = np.zeros((K, 7))
        poses[:, 0] = 0.3 * np.arange(K)
        yaw = 0.002 * np.arange(K)
        poses[:, 3], poses[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        ids = np.arange(K)
        p32 = [lom.Pose3D(p[:3].astype(np.float32), p[3:].astype(np.float32)) for p in poses]
        g = lom.VoxelGrid(float(np.float32(0.2)), 20)
        sizes = {}

        def assemble(cull):
            g.setVoxelSize(float(np.float32(0.2)))
            g.size()
            t0 = time.perf_counter()
            st = g.assemble(arch, ids, poses, centre=poses[-1, :3] if cull else None, radius=80.0 if cull else 0.0)
            g.size()
            dt = time.perf_counter() - t0
            sizes["assemble_cull" if cull else "assemble"] = (st["points_kept"], st["voxels_after"])
            return dt * 1e3

        def per_scan():
            g.setVoxelSize(float(np.float32(0.2)))
            g.size()
            ox, on = C.c_void_p(), C.c_void_p()
            t0 = time.perf_counter()
            for k in range(K):
                dx, dn = dev[k % args.distinct]
                capi.check(L.lom_transform_points_device(g.handle, C.byref(p32[k]._c()), dx.data_ptr(), dn.data_ptr(), len(dx), 12,
                                                         C.byref(ox), C.byref(on)), g.handle)
                capi.check(L.lom_map_add_points_device(g.handle, ox, on, len(dx), 12), g.handle)
            n = g.size()
            dt = time.perf_counter() - t0
            sizes["per_scan"] = (g.pointCount(), n)
            return dt * 1e3

        kinds = {"assemble_ms": lambda: assemble(False), "assemble_cull_ms": lambda: assemble(True), "per_scan_ms": per_scan}
        names = list(kinds)
        calls = args.calls if K < 64 else 1
        for fn in kinds.values():
            fn()  # warm-up: buffers, code objects
        per_block = {k: [] for k in names}
        for b in range(args.blocks):
            for k in (names if b % 2 == 0 else names[::-1]):
                per_block[k].append(statistics.median([kinds[k]() for _ in range(calls)]))
        rec = {k: _spread(v) for k, v in per_block.items()}
        rec["points_in"] = int(arch.pointCount())
        rec["kept_and_voxels"] = sizes
        out["K"][str(K)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
