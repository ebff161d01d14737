#!/usr/bin/env python3
"""Throughput of the batched quality report: one JSON line, also written to profiles/quality_batch_throughput.json.

The C2 problem of bench.py (bench.build_workload(1, 0): the VLP16 scan against the 500k-point map), the scan resident in
HBM, scored with the full scan and with every 4th point (stride_bytes * 4, n / 4) at K in {1, 8, 64, 512, 4096} poses
taken evenly from a lom_pose_lattice of +-1 m (0.1 m) by +-10 degrees (2 degrees) around the pose the align returns.
    batch     one lom_match_quality_batch_sums_device call for the K poses
    singles   K calls of lom_match_quality_device on the same handle, in the same process
Both are called from Python through ctypes with the argument structures built beforehand; blocks of the two alternate
(--blocks of each, at least five), a block repeats its measurement until it has scored --poses-per-block poses, and the
per-block wall times per K poses are reported with their range.
    python tools/quality_batch_throughput.py [--blocks 5] [--poses-per-block 256]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KS = (1, 8, 64, 512, 4096)


def _spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--poses-per-block", type=int, default=256)
    args = ap.parse_args()
    blocks = max(5, args.blocks)
    import torch

    import bench
    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi

    L = capi.lib()
    work = bench.build_workload(1, 0)
    grid = lom.VoxelGrid(0.5, 20)
    grid.addCloud(work["map_xyz"], work["map_nrm"])
    scan = torch.from_numpy(np.ascontiguousarray(work["scan"], np.float32)).to("cuda:0")
    torch.cuda.synchronize()
    n = int(scan.shape[0])
    centre = lom.CloudMatcher().alignDevice(grid, scan.data_ptr(), n, lom.Pose3D())
    # (half a step of slack: 1.0f / 0.1f and 10 / 2 degrees in f32 fall just below a whole number of steps)
    lattice = lom.pose_lattice(centre, (1.05, 1.05, 0.0), (0.1, 0.1, 0.0), math.radians(11.0), math.radians(2.0))
    assert len(lattice) >= max(KS), len(lattice)
    rep = capi.QualityReport()
    out = {"device": torch.cuda.get_device_name(0), "config": "C2", "points": n, "lattice_nodes": len(lattice),
           "blocks_each": blocks,
           "commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None,
           "note": "wall time per K poses incl. the ctypes calls; medians and ranges over alternating blocks",
           "clouds": {}}
    for name, every in (("full_scan", 1), ("every_4th_point", 4)):
        nn, stride = n // every, 12 * every
        rows = {}
        for K in KS:
            pick = [len(lattice) // 2] if K == 1 else [int(round(v)) for v in np.linspace(0, len(lattice) - 1, K)]
            poses = [lattice[i] for i in pick]
            problems = lom.quality_problems([(scan.data_ptr(), nn, stride, p) for p in poses])
            sums = np.zeros((K, capi.NQSUMS))
            sums_p = sums.ctypes.data_as(C.POINTER(C.c_double))
            singles = [(capi.f3(p.translation), capi.f4(p.rotation)) for p in poses]

            def batch():
                capi.check(L.lom_match_quality_batch_sums_device(grid.handle, problems, K, 0.3, sums_p), grid.handle)

            def single_calls():
                for t3, q4 in singles:
                    capi.check(L.lom_match_quality_device(grid.handle, scan.data_ptr(), nn, stride, t3, q4, 0.3, 0.0, 0.0,
                                                          C.byref(rep), None), grid.handle)

            reps = max(1, args.poses_per_block // K)
            batch()
            single_calls() if K <= 512 else None
            valid_single = int(rep.valid)
            us = {"batch": [], "singles": []}
            for b in range(blocks):
                for key, fn in ((("batch", batch), ("singles", single_calls)) if b % 2 == 0 else
                                (("singles", single_calls), ("batch", batch))):
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        fn()
                    us[key].append((time.perf_counter() - t0) / reps * 1e6)
            assert int(sums[K - 1, 33]) == int(rep.valid), (int(sums[K - 1, 33]), int(rep.valid), valid_single)
            mb, ms = statistics.median(us["batch"]), statistics.median(us["singles"])
            rows[str(K)] = {"batch_us_per_call": _spread(us["batch"]), "singles_us_per_K_calls": _spread(us["singles"]),
                            "batch_poses_per_s": round(K / mb * 1e6, 1), "singles_poses_per_s": round(K / ms * 1e6, 1),
                            "singles_over_batch": round(ms / mb, 3), "calls_per_block": reps,
                            "best_valid": int(sums[:, 33].max())}
        out["clouds"][name] = {"points_scored": nn, "stride_bytes": stride, "K": rows}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "quality_batch_throughput.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
