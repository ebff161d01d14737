#!/usr/bin/env python3
"""What ray carving costs on the streaming workload (C5: the 10 Hz VLP16 sequence, default parameters): one JSON line.
    carve_us          lom_map_carve_rays_device of one frame's update cloud (in HBM, map frame) against the C5 keyframe,
                      enqueue to the end of its back half, by HIP events on the map's stream; the keyframe is rebuilt
                      from its export before every call (outside the events), so that every call erases what the first
                      one does
    radius_cleanup_us lom_map_radius_cleanup on the same map at the same pose and the pipeline's 80 m, likewise
                      both in --blocks alternating blocks of --calls calls: median and spread of the block medians
    frame_ms          lom_odometry_process_cloud per frame over --frames frames with carve unset and set, alternating
                      blocks (a fresh odometry per block, wall clock over the block)
    The split of k_carve_hits / k_carve_walk / k_carve_flag comes from a run of its own:
        rocprofv3 --kernel-trace --stats -- python tools/carve_cost.py --blocks 1 --frames 0
    python tools/carve_cost.py [--calls 20] [--blocks 5] [--frame 60] [--frames 100] > profiles/carve_cost.json
The defaults against the parent commit: tools/ab_trees.sh -> profiles/carve_ab.txt."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs, digits=2):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frame", type=int, default=60, help="the frame whose update cloud is carved; the keyframe is that of the frames before it")
    ap.add_argument("--frames", type=int, default=100, help="frames per block of the frame-time comparison (0: skip it)")
    ap.add_argument("--margin", type=float, default=0.4)
    ap.add_argument("--min-range", type=float, default=4.0)
    ap.add_argument("--max-range", type=float, default=80.0)
    ap.add_argument("--min-crossings", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi, synth

    L = capi.lib()
    params = dict(margin=args.margin, min_range=args.min_range, max_range=args.max_range, min_crossings=args.min_crossings)
    boxes = synth.make_boxes()
    n_seq = max(args.frame + 1, args.frames)
    frames = [synth.make_sequence_frame(k, boxes=boxes) for k in range(n_seq)]
    torch.zeros(1, device="cuda:0")

    # the C5 keyframe before frame `--frame`, and that frame's update cloud as the pipeline makes it
    od = lom.LidarOdometry()
    for k in range(args.frame):
        od.processCloud(frames[k])
    key_xyz, key_nrm = od.getFullKeyFrameCloudWithNormals()
    od.processCloud(frames[args.frame])
    pose = od.getCurrentPose()
    pxyz, pnrm, _, _ = lom.classify(od.getTempCloud())
    fx, fn = lom.rangeFilter(pxyz, pnrm, od.params.lidar_min_range, od.params.lidar_max_range)
    dx, _ = lom.VoxelGrid(0.5, 1).downsample(fx, fn, od.params.keyframe_update_voxel_size)
    rays = np.ascontiguousarray(lom.transform_points(pose, dx), np.float32)
    d_rays = torch.from_numpy(rays).cuda()
    origin = capi.f3(pose.translation)
    cleanup_range = float(od.params.keyframe_cleanup_range)
    del od

    g = lom.VoxelGrid(float(np.float32(0.2)), 20)
    stream = torch.cuda.ExternalStream(L.lom_map_get_stream(g.handle))
    p = lom.carveParams(params)
    stats = capi.CarveStats()
    last = {}

    def rebuild():
        g.setVoxelSize(float(np.float32(0.2)))
        g.addCloud(key_xyz, key_nrm)
        g.size()  # settles the insert: nothing of it is left on the stream

    def one(what):
        rebuild()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if what == "carve":
            capi.check(L.lom_map_carve_rays_device(g.handle, origin, d_rays.data_ptr(), len(rays), 12, C.byref(p),
                                                   C.byref(stats)), g.handle)
            last["stats"] = stats.asdict()
        else:
            capi.check(L.lom_map_radius_cleanup(g.handle, origin, cleanup_range), g.handle)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    kinds = ("carve", "radius_cleanup")
    per_block = {k: [] for k in kinds}
    for k in kinds:  # warm-up: scratch, code objects
        for _ in range(3):
            one(k)
    for b in range(args.blocks):
        for k in (kinds if b % 2 == 0 else kinds[::-1]):
            per_block[k].append(statistics.median([one(k) for _ in range(args.calls)]))
    rebuild()
    out = {"device": torch.cuda.get_device_name(0), "frame": args.frame, "rays": len(rays), "keyframe_voxels": g.size(),
           "params": params, "carve_stats": last.get("stats"),
           "note": "us per call, HIP events on the map's stream around the call (includes its one read-back)",
           "carve_us": _spread(per_block["carve"]), "radius_cleanup_us": _spread(per_block["radius_cleanup"])}

    if args.frames > 0:
        def block(carve):
            o = lom.LidarOdometry()
            if carve:
                o.setCarve(params)
            o.processCloud(frames[0])
            t0 = time.perf_counter()
            for k in range(1, args.frames):
                o.processCloud(frames[k])
            o.stats  # waits for the last keyframe update
            return (time.perf_counter() - t0) / (args.frames - 1) * 1e3, o.getCurrentPose().translation.tolist()

        ms = {"unset": [], "set": []}
        block(False)
        block(True)
        for b in range(args.blocks):
            for name in (("unset", "set") if b % 2 == 0 else ("set", "unset")):
                t, where = block(name == "set")
                ms[name].append(t)
                out["final_translation_" + name] = where
        out["frame_ms"] = {k: _spread(vs, 4) for k, vs in ms.items()}
        out["frames_per_block"] = args.frames
    print(json.dumps(out))


if __name__ == "__main__":
    main()
