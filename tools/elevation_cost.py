#!/usr/bin/env python3
"""What the elevation grid costs: one JSON line.
The full scans of tools/occupancy_cost.py along its slow drive (x = 0.3 k, a small yaw): the whole time-normalised frame,
about 26.6k points, K in --scans, repeated round robin from --distinct synthetic frames (synth.make_sequence_frame), into
grids of --resolutions that hold the drive and the range around it.  Band -3 .. 1 m around the sensor, range 2-60 m.  Per
(K, resolution), in --blocks alternating blocks (one call per block and variant), HIP events on the grid's stream around
the call -- from its enqueue to the end of its read-back -- medians and ranges of the block values:
    merge_ms      lom_elevation_integrate as the library ships it: the lanes of a wave that share a cell merged first
    no_merge_ms   the same call with LOM_ELEV_OPT_TEST_WAVE_MERGE = 0: four atomics per contributing point
both into a cleared grid, in the same process: the pair tells whether the wave merge pays.  points_per_ms is the call's
points over the median.  cost_ms: lom_elevation_cost on the grid so filled (min_points 2, R = 2), read-back included.
odometry_scan_ms: lom_odometry_elevation_scan per frame over --frames frames of bench.py's C5 drive
(synth.make_sequence_frame with synth.make_boxes).
    python tools/elevation_cost.py [--scans 16,128,512] [--blocks 5] > profiles/elevation_cost.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", default="16,128,512")
    ap.add_argument("--resolutions", default="0.25,0.1")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic frames behind the K scans")
    ap.add_argument("--frames", type=int, default=20, help="frames of the odometry drive (0: none)")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi, synth

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    clouds = []
    for k in range(args.distinct):
        frame = lom.pointTimeNormalize(synth.make_sequence_frame(k * 10))
        clouds.append(np.ascontiguousarray(np.stack([frame["x"], frame["y"], frame["z"]], 1), np.float32))
    pts = dict(z_lo=-3.0, z_hi=1.0, min_range=2.0, max_range=60.0)
    layer, cost = dict(min_points=2, window=2), dict(max_slope=0.35, max_step=0.25, max_rough=0.1, max_span=0.5)
    out = {"device": torch.cuda.get_device_name(0), "point_params": pts, "layer_params": layer, "cost_params": cost,
           "points_per_scan": [len(x) for x in clouds],
           "note": "ms per call, HIP events on the grid's stream, read-back included; each integrate into a cleared grid", "runs": []}

    def timed(stream, settle, fn):
        settle()  # nothing of the call before is left on the stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for K in [int(s) for s in args.scans.split(",")]:
        arch = lom.ScanArchive(sum(len(clouds[k % args.distinct]) for k in range(K)), K)
        for k in range(K):
            arch.addPoints(clouds[k % args.distinct])
        poses = np.zeros((K, 7))
        poses[:, 0] = 0.3 * np.arange(K)
        yaw = 0.002 * np.arange(K)
        poses[:, 3], poses[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        ids = np.arange(K)
        for res in [float(s) for s in args.resolutions.split(",")]:
            width, height = min(int((0.3 * K + 140.0) / res), 8192), int(40.0 / res)
            g = lom.ElevationGrid(res, (-70.0, -20.0), width, height, 0.0)
            stream = torch.cuda.ExternalStream(L.lom_elevation_stream(g.handle))
            seen = {}

            def integrate(merge):
                g.setOption(capi.ELEV_OPT_TEST_WAVE_MERGE, merge)
                return timed(stream, g.clear, lambda: seen.__setitem__("stats", g.integrate(arch, ids, poses, pts)))

            def costed():
                return timed(stream, lambda: g.cells(), lambda: seen.__setitem__("summary", g.cost(layer, cost)[1]))

            rec = {"K": K, "resolution": res, "width": width, "height": height, "points_in": int(arch.pointCount())}
            kinds = {"merge_ms": lambda: integrate(-1), "no_merge_ms": lambda: integrate(0)}
            names = list(kinds)
            for fn in kinds.values():
                fn()  # warm-up: buffers, code objects
            per_block = {k: [] for k in names}
            for b in range(args.blocks):
                for k in (names if b % 2 == 0 else names[::-1]):
                    per_block[k].append(kinds[k]())
            rec.update({k: _spread(v) for k, v in per_block.items()})
            rec["stats"] = seen["stats"]
            rec["points_per_ms"] = {k: round(seen["stats"]["points"] / statistics.median(v), 1) for k, v in per_block.items()}
            costed()
            rec["cost_ms"] = _spread([costed() for _ in range(args.blocks)])
            rec["summary"] = seen["summary"]
            out["runs"].append(rec)
    if args.frames:
        boxes = synth.make_boxes()
        o = lom.LidarOdometry()
        g = lom.ElevationGrid(0.25, (-70.0, -20.0), 800, 160, 0.0)
        stream = torch.cuda.ExternalStream(L.lom_elevation_stream(g.handle))
        ms, seen = [], {}
        for k in range(args.frames):
            o.processCloud(synth.make_sequence_frame(k, boxes=boxes))
            dt = timed(stream, lambda: g.cells(), lambda: seen.__setitem__("stats", o.elevationScan(g, pts)))
            if k >= 2:  # (the first calls allocate)
                ms.append(dt)
        out["odometry_scan_ms"] = dict(_spread(ms), resolution=0.25, last_stats=seen["stats"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
