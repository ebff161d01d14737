#!/usr/bin/env python3
"""Batched align throughput on C2 (bench.build_workload(1, 0): the VLP16 scan against the 500k-point map): one JSON line.
For K in {1, 2, 4, 8, 16} problems, two forms -- the same scan from K seeded guesses within 0.1 m / 1 deg ("same_scan"),
and K different scans ("different_scans") -- it reports
    batch_ms      median over --calls lom_match_align_batch_device calls (after warm-up), the Python call included
    aligns_per_s  K / batch_ms
    seq_ms        the same K problems as K single aligns issued from compiled code (lom_match_align_repeat, `--reps`
                  back to back per problem, divided): what one caller does without the batch
    rounds        device rounds the batch used
    python tools/batch_throughput.py [--calls 200] [--warmup 20] [--reps 50] [--ks 1,2,4,8,16] [--forms same_scan,...]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--forms", default="same_scan,different_scans")
    args = ap.parse_args()
    import torch

    import bench
    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import synth

    work = bench.build_workload(1, 0)
    grid = lom.VoxelGrid(0.5, 20)
    grid.addCloud(work["map_xyz"], work["map_nrm"])
    ks = [int(k) for k in args.ks.split(",")]
    kmax = max(ks)
    rng = np.random.default_rng(2024)
    deg = np.pi / 180.0
    guesses = []
    for _ in range(kmax):
        t = rng.uniform(-0.1, 0.1, 3) / np.sqrt(3.0)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = float(rng.uniform(-1.0, 1.0)) * deg
        guesses.append(lom.Pose3D(t, (np.cos(a / 2), *(np.sin(a / 2) * axis))))
    scan = torch.from_numpy(np.ascontiguousarray(work["scan"], np.float32)).to("cuda:0")
    boxes = synth.make_boxes()
    scans = [scan]
    for k in range(1, kmax):  # the same scene seen from poses a few centimetres apart, own sensor noise each
        s, _, _, _ = synth.make_scan(16, 1800, true_t=(0.10 + 0.01 * k, -0.05, 0.02), seed_noise=1000 + k, boxes=boxes)
        scans.append(torch.from_numpy(np.ascontiguousarray(s, np.float32)).to("cuda:0"))
    torch.cuda.synchronize()
    m = lom.CloudMatcher()
    out = {"config": "C2", "name": work["name"], "device": torch.cuda.get_device_name(0),
           "note": "batch_ms: median of per-call wall times incl. the Python call; seq_ms: K single aligns from compiled "
                   "code (lom_match_align_repeat)", "forms": {}}
    for form in args.forms.split(","):
        rows = []
        for k in ks:
            if form == "same_scan":
                items = [(scan.data_ptr(), scan.shape[0], guesses[i]) for i in range(k)]
            else:
                items = [(scans[i].data_ptr(), scans[i].shape[0], lom.Pose3D()) for i in range(k)]
            for _ in range(args.warmup):
                m.alignBatchDevice(grid, items)
            times = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                m.alignBatchDevice(grid, items)
                times.append(time.perf_counter() - t0)
            rounds = max(s["round"] for s in m.batch_stats) + 1
            fallbacks = sum(s["host_fallback"] for s in m.batch_stats)
            batch_ms = statistics.median(times) * 1e3
            seq_s = 0.0
            for ptr, n, g in items:
                lom.align_repeat(grid, ptr, n, g, 5)
                t0 = time.perf_counter()
                lom.align_repeat(grid, ptr, n, g, args.reps)
                seq_s += (time.perf_counter() - t0) / args.reps
            rows.append({"K": k, "batch_ms": round(batch_ms, 4), "aligns_per_s": round(k / batch_ms * 1e3, 1),
                         "seq_ms": round(seq_s * 1e3, 4), "seq_aligns_per_s": round(k / seq_s, 1),
                         "speedup": round(seq_s * 1e3 / batch_ms, 3), "rounds": rounds, "host_fallbacks": fallbacks,
                         "outer_iterations": [s["outer_iterations"] for s in m.batch_stats]})
            print(f"[batch_throughput] {form} K={k}: {rows[-1]}", file=sys.stderr)
        out["forms"][form] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
