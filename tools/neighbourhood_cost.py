#!/usr/bin/env python3
"""What the neighbourhood classifier costs on a C5 frame (28.8k points): one JSON line.
    front_end_us   lom_frontend_process of one frame, enqueue to last kernel, by HIP events on the front end's stream:
                   the ring classifier (k_fe_stats, k_fe_deskew, k_fe_curv, k_fe_planar) and the neighbourhood classifier
                   (k_fe_stats, k_fe_deskew, index clear + insert, k_nb_eval, k_nb_compact) on the same frame from the
                   same process, in --blocks alternating blocks of --calls frames; median and spread of the block medians
    The per-kernel split comes from one `rocprofv3 --kernel-trace --stats -- python tools/neighbourhood_cost.py --blocks 1`.
    python tools/neighbourhood_cost.py [--calls 40] [--blocks 5] [--frame 50]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frame", type=int, default=50)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--index-cap", type=int, default=64)
    args = ap.parse_args()
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi, synth

    L = capi.lib()
    frame = synth.make_sequence_frame(args.frame)
    params = dict(radius=args.radius, index_cap=args.index_cap, min_neighbours=8, max_variation=0.01, min_spread=0.02)
    torch.zeros(1, device="cuda:0")
    fe = lom.FrontEnd()
    L.lom_frontend_stream.restype = C.c_void_p
    stream = torch.cuda.ExternalStream(L.lom_frontend_stream(fe._h))
    start, end = lom.Pose3D((0.05, -0.02, 0.01), synth.quat_from_ypr(0.6, 0.1, -0.05)), lom.Pose3D()
    counts = (C.c_uint32 * 4)()
    found = {}

    def one(kind):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fe._check(L.lom_frontend_process(fe._h, frame.ctypes.data, len(frame), C.byref(start._c()), C.byref(end._c()), 4.0, 80.0))
        e1.record(stream)
        fe._check(L.lom_frontend_wait(fe._h, counts))
        found[kind] = (int(counts[0]), int(counts[1]))
        return e0.elapsed_time(e1) * 1e3

    kinds = (("rings", capi.CLASSIFIER_RINGS, None), ("neighbourhood", capi.CLASSIFIER_NEIGHBOURHOOD, params))
    per_block = {k: [] for k, _, _ in kinds}
    for name, kind, p in kinds:  # warm-up: buffers, the index workspace, code objects
        fe.setClassifier(kind, p)
        for _ in range(5):
            one(name)
    for b in range(args.blocks):
        for name, kind, p in (kinds if b % 2 == 0 else kinds[::-1]):
            fe.setClassifier(kind, p)
            one(name)
            per_block[name].append(statistics.median([one(name) for _ in range(args.calls)]))
    out = {"device": torch.cuda.get_device_name(0), "points": len(frame), "params": params,
           "note": "us per frame, HIP events around lom_frontend_process (includes the pinned-host read of the frame)",
           "front_end_us": {k: _spread(v) for k, v in per_block.items()},
           "planar_filtered": {k: list(v) for k, v in found.items()}, "redos": fe.debugCounter()}
    out["added_us_median"] = round(out["front_end_us"]["neighbourhood"]["median"] - out["front_end_us"]["rings"]["median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
