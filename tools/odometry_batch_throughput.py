#!/usr/bin/env python3
"""Batched odometry throughput: K independent LiDAR streams, each its own synthetic world (synth.make_boxes(seed)) driven
through synth.make_sequence_frame, stepped three ways after --warmup frames.  One JSON line.
    batch     LidarOdometry.processBatch: one call per step for all K streams (one multi-map align)
    seq       the same K handles stepped one after another with processCloud from one thread
    threads   K threads, each stepping its own handle with processCloud
For each: ms per step (K frames; wall time of --steps steps including the last keyframe update, divided) and aggregate
frames/s.  Fresh handles per form and K; LOM_HOST_THREADS (--host-threads) is the same for every form.
    python tools/odometry_batch_throughput.py [--ks 1,2,4,8,16] [--steps 30] [--warmup 5] [--host-threads 1]"""
import argparse
import gc
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _frames(job):
    """frames `first` .. `first + count - 1` of the sequence in world `seed`"""
    from lidar_odometry_demo_amd import synth

    seed, first, count = job
    boxes = synth.make_boxes(seed)
    return [synth.make_sequence_frame(first + f, boxes=boxes) for f in range(count)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=1)
    ap.add_argument("--forms", default="batch,seq,threads")
    args = ap.parse_args()
    os.environ["LOM_HOST_THREADS"] = str(args.host_threads)  # read by lom_odometry_create
    import lidar_odometry_demo_amd as lom

    ks = [int(k) for k in args.ks.split(",")]
    kmax = max(ks)
    n_frames = args.warmup + args.steps
    # stream j: world seed 500 + j, frames from 3 j on (different worlds and phases of the motion)
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor

    with ProcessPoolExecutor(max_workers=min(8, kmax), mp_context=mp.get_context("spawn")) as ex:
        frames = list(ex.map(_frames, [(500 + j, 3 * j, n_frames) for j in range(kmax)]))
    points = sum(len(f) for s in frames for f in s) / (kmax * n_frames)

    def settle(odos):
        for o in odos:
            _ = o.stats  # joins the last deferred keyframe update

    def run(form, k):
        odos = [lom.LidarOdometry() for _ in range(k)]
        if form == "batch":
            def step(f):
                lom.LidarOdometry.processBatch(odos, [frames[j][f] for j in range(k)])
            for f in range(args.warmup):
                step(f)
            settle(odos)
            t0 = time.perf_counter()
            for f in range(args.warmup, n_frames):
                step(f)
            settle(odos)
            wall = time.perf_counter() - t0
        elif form == "seq":
            for f in range(args.warmup):
                for j in range(k):
                    odos[j].processCloud(frames[j][f])
            settle(odos)
            t0 = time.perf_counter()
            for f in range(args.warmup, n_frames):
                for j in range(k):
                    odos[j].processCloud(frames[j][f])
            settle(odos)
            wall = time.perf_counter() - t0
        else:
            errors = []
            start = threading.Barrier(k + 1)

            def work(j):
                try:
                    for f in range(args.warmup):
                        odos[j].processCloud(frames[j][f])
                    settle([odos[j]])
                    start.wait()
                    for f in range(args.warmup, n_frames):
                        odos[j].processCloud(frames[j][f])
                    settle([odos[j]])
                except Exception as e:  # noqa: BLE001 -- reported below
                    errors.append(repr(e))
                    start.abort()

            th = [threading.Thread(target=work, args=(j,)) for j in range(k)]
            for t in th:
                t.start()
            start.wait()
            t0 = time.perf_counter()
            for t in th:
                t.join()
            wall = time.perf_counter() - t0
            if errors:
                raise RuntimeError(errors[0])
        poses = [o.getCurrentPose() for o in odos]
        del odos
        gc.collect()
        return wall, poses

    rows = []
    for k in ks:
        row = {"k": k}
        ref = None
        for form in args.forms.split(","):
            wall, poses = run(form, k)
            row[f"{form}_ms_per_step"] = round(wall / args.steps * 1e3, 4)
            row[f"{form}_frames_per_s"] = round(k * args.steps / wall, 1)
            bits = [p.translation.tobytes() + p.rotation.tobytes() for p in poses]
            if ref is None:
                ref = bits
            row[f"{form}_same_poses"] = bits == ref
        if "batch_frames_per_s" in row and "seq_frames_per_s" in row:
            row["batch_over_seq"] = round(row["batch_frames_per_s"] / row["seq_frames_per_s"], 3)
        rows.append(row)
    import torch

    print(json.dumps({"tool": "odometry_batch_throughput", "device": torch.cuda.get_device_name(0),
                      "points_per_frame": round(points, 1), "steps": args.steps, "warmup": args.warmup,
                      "host_threads": args.host_threads, "rows": rows}))


if __name__ == "__main__":
    main()
