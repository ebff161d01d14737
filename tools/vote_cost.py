#!/usr/bin/env python3
"""What the scan votes cost beside the calls around them: one JSON line.
Synthetic scans (synth.make_sequence_frame: classify, range filter, down-sampling at the update voxel size; about 8k
points each, repeated round robin to K) along a slow drive, K in --scans, into a map of voxel 0.5 / 20 points per voxel.
Per K, in --blocks alternating blocks (one call per block and variant), HIP events on the map's stream around the
call -- from its enqueue to the end of its back half, its read-backs included -- medians and ranges of the block values:
    assemble_ms      lom_map_assemble of the K scans into the cleared map (the map every other variant starts from)
    carve_scans_ms   lom_map_carve_scans of the same scans at the same poses on that map (the parameters of
                     tests/vote_scene.py: margin 0.4, range 4-60 m, clearance 0.75, 3 free scans, 2 per seen vote)
    carve_rays_ms    the yardstick: K calls of lom_map_carve_rays_device on the same rays (the scans transformed on the
                     host beforehand, in HBM; margin and range as above, min_crossings 2) on that map -- another rule
                     and other erasures, the same walks but for the clearance
--trace: nothing is timed; one assemble and one carve_scans per K, for `rocprofv3 --kernel-trace --stats -- python
tools/vote_cost.py --trace --scans 128` in a run of its own.
    python tools/vote_cost.py [--scans 16,128,512] [--blocks 5] > profiles/vote_cost.json"""
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
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic frames behind the K scans")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi, synth
    from tests import assemble_ref

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    prm = lom.LidarOdometry().params
    ws = lom.VoxelGrid(0.5, 1)
    clouds = []
    for k in range(args.distinct):
        pxyz, pnrm, _, _ = lom.classify(lom.pointTimeNormalize(synth.make_sequence_frame(k * 10)))
        fx, fn = lom.rangeFilter(pxyz, pnrm, prm.lidar_min_range, prm.lidar_max_range)
        clouds.append(ws.downsample(fx, fn, prm.keyframe_update_voxel_size))
    votes = dict(margin=0.4, min_range=4.0, max_range=60.0, clearance=0.75, min_free_scans=3, free_per_seen=2)
    carve = dict(margin=0.4, min_range=4.0, max_range=60.0, min_crossings=2)
    out = {"device": torch.cuda.get_device_name(0), "points_per_scan": [len(x) for x, _ in clouds], "voxel": 0.5,
           "max_points": 20, "vote_params": votes, "carve_params": carve,
           "note": "ms per call (carve_rays_ms: per K calls), HIP events on the map's stream, read-backs included", "K": {}}
    for K in [int(s) for s in args.scans.split(",")]:
        arch = lom.ScanArchive(sum(len(clouds[k % args.distinct][0]) for k in range(K)), K)
        for k in range(K):
            arch.add(*clouds[k % args.distinct])
        poses = np.zeros((K, 7))  # a slow drive along x with a small yaw, as the sequence's
        poses[:, 0] = 0.3 * np.arange(K)
        yaw = 0.002 * np.arange(K)
        poses[:, 3], poses[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        ids = np.arange(K)
        g = lom.VoxelGrid(0.5, 20)
        stream = torch.cuda.ExternalStream(L.lom_map_get_stream(g.handle))
        seen = {}

        def timed(fn):
            g.size()  # settled: nothing of the call before is left on the stream
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def assemble():
            g.setVoxelSize(0.5)  # cleared
            dt = timed(lambda: seen.__setitem__("assemble", g.assemble(arch, ids, poses)))
            return dt

        def carve_scans():
            assemble()
            return timed(lambda: seen.__setitem__("carve_scans", g.carveScans(arch, ids, poses, votes)))

        if args.trace:
            carve_scans()
            out["K"][str(K)] = seen
            continue
        rays = []
        for k in range(K):
            x, _ = assemble_ref.transform(poses[k], *clouds[k % args.distinct])
            rays.append((torch.from_numpy(x).cuda(), poses[k, :3].astype(np.float32)))
        torch.cuda.synchronize()

        def carve_rays():
            assemble()
            erased = [0]

            def run():
                for d, o in rays:
                    erased[0] += g.carveRays(o, None, carve, device_ptr=d.data_ptr(), n=len(d))["voxels_erased"]

            dt = timed(run)
            seen["carve_rays_voxels_erased"] = erased[0]
            return dt

        kinds = {"assemble_ms": assemble, "carve_scans_ms": carve_scans, "carve_rays_ms": carve_rays}
        names = list(kinds)
        for fn in kinds.values():
            fn()  # warm-up: buffers, code objects
        per_block = {k: [] for k in names}
        for b in range(args.blocks):
            for k in (names if b % 2 == 0 else names[::-1]):
                per_block[k].append(kinds[k]())
        rec = {k: _spread(v) for k, v in per_block.items()}
        rec["points_in"] = int(arch.pointCount())
        rec["results"] = seen
        out["K"][str(K)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
