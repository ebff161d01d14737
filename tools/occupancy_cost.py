#!/usr/bin/env python3
"""What the occupancy grid costs: one JSON line.
Two kinds of scan along a slow drive (x = 0.3 k, a small yaw), K in --scans, repeated round robin from --distinct synthetic
frames (synth.make_sequence_frame):
    update   tools/vote_cost.py's scans: classify, range filter, down-sampling at the update voxel size (about 8k points)
    full     the whole time-normalised frame, about 26.6k points: what lom_odometry_archive_deskewed stores
into grids of --resolutions that hold the drive and the range around it.  The parameters are those of
tests/occupancy_scene.py (band -1.5 .. 0.6 m, margin 0, range 2-60 m).  Per (kind, K, resolution), in --blocks
alternating blocks (one call per block and variant), HIP events on the grid's stream around the call -- from its enqueue to
the end of its read-back -- medians and ranges of the block values:
    window_default_ms   lom_occupancy_integrate with the LDS window the library ships (512 cells a side)
    window_0_ms         the same call with LOM_OCC_OPT_TEST_WINDOW = 0: every pass bit goes to global memory
both into a cleared grid, in the same process: the pair tells whether the LDS window pays.  cells_per_ms is cells_visited
of the call over the median.  odometry_scan_ms: lom_odometry_occupancy_scan per frame over --frames frames of a drive.
--trace: nothing is timed; one integrate per (kind, K, resolution), for `rocprofv3 --kernel-trace --stats -- python
tools/occupancy_cost.py --trace --scans 128` in a run of its own.
    python tools/occupancy_cost.py [--scans 16,128,512] [--blocks 5] > profiles/occupancy_cost.json"""
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
    ap.add_argument("--kinds", default="update,full")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic frames behind the K scans")
    ap.add_argument("--frames", type=int, default=20, help="frames of the odometry drive (0: none)")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi, synth

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    prm = lom.LidarOdometry().params
    ws = lom.VoxelGrid(0.5, 1)
    clouds = {"update": [], "full": []}
    for k in range(args.distinct):
        frame = lom.pointTimeNormalize(synth.make_sequence_frame(k * 10))
        pxyz, pnrm, _, _ = lom.classify(frame)
        fx, fn = lom.rangeFilter(pxyz, pnrm, prm.lidar_min_range, prm.lidar_max_range)
        clouds["update"].append(ws.downsample(fx, fn, prm.keyframe_update_voxel_size)[0])
        clouds["full"].append(np.ascontiguousarray(np.stack([frame["x"], frame["y"], frame["z"]], 1), np.float32))
    rays = dict(z_lo=-1.5, z_hi=0.6, margin=0.0, min_range=2.0, max_range=60.0)
    out = {"device": torch.cuda.get_device_name(0), "ray_params": rays,
           "points_per_scan": {k: [len(x) for x in v] for k, v in clouds.items()},
           "note": "ms per call, HIP events on the grid's stream, read-back included; each call into a cleared grid", "runs": []}

    def timed(stream, settle, fn):
        settle()  # nothing of the call before is left on the stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for kind in args.kinds.split(","):
        for K in [int(s) for s in args.scans.split(",")]:
            src = clouds[kind]
            arch = lom.ScanArchive(sum(len(src[k % args.distinct]) for k in range(K)), K)
            for k in range(K):
                arch.addPoints(src[k % args.distinct])
            poses = np.zeros((K, 7))
            poses[:, 0] = 0.3 * np.arange(K)
            yaw = 0.002 * np.arange(K)
            poses[:, 3], poses[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
            ids = np.arange(K)
            for res in [float(s) for s in args.resolutions.split(",")]:
                width, height = int((0.3 * K + 140.0) / res), int(40.0 / res)
                g = lom.OccupancyGrid(res, (-70.0, -20.0), width, height)
                stream = torch.cuda.ExternalStream(L.lom_occupancy_stream(g.handle))
                seen = {}

                def integrate(window):
                    g.setOption(capi.OCC_OPT_TEST_WINDOW, window)
                    return timed(stream, g.clear, lambda: seen.__setitem__("stats", g.integrate(arch, ids, poses, rays)))

                rec = {"kind": kind, "K": K, "resolution": res, "width": width, "height": height,
                       "points_in": int(arch.pointCount())}
                if args.trace:
                    integrate(-1)
                    rec["stats"] = seen["stats"]
                    out["runs"].append(rec)
                    continue
                kinds = {"window_default_ms": lambda: integrate(-1), "window_0_ms": lambda: integrate(0)}
                names = list(kinds)
                for fn in kinds.values():
                    fn()  # warm-up: buffers, code objects
                per_block = {k: [] for k in names}
                for b in range(args.blocks):
                    for k in (names if b % 2 == 0 else names[::-1]):
                        per_block[k].append(kinds[k]())
                rec.update({k: _spread(v) for k, v in per_block.items()})
                rec["stats"] = seen["stats"]
                rec["cells_per_ms"] = {k: round(seen["stats"]["cells_visited"] / statistics.median(v), 1) for k, v in per_block.items()}
                _, summary = g.classify(dict(min_free_scans=3, free_per_seen=2, min_seen_scans=1))
                rec["summary"] = summary
                out["runs"].append(rec)
    if args.frames and not args.trace:
        o = lom.LidarOdometry()
        g = lom.OccupancyGrid(0.25, (-70.0, -20.0), 800, 160)
        stream = torch.cuda.ExternalStream(L.lom_occupancy_stream(g.handle))
        ms, seen = [], {}
        for k in range(args.frames):
            o.processCloud(synth.make_sequence_frame(k))
            dt = timed(stream, lambda: g.counts(), lambda: seen.__setitem__("stats", o.occupancyScan(g, rays)))
            if k >= 2:  # (the first calls allocate)
                ms.append(dt)
        out["odometry_scan_ms"] = dict(_spread(ms), resolution=0.25, last_stats=seen["stats"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
