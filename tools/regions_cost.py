#!/usr/bin/env python3
"""What the region grid costs: one JSON line.
lom_regions_extract_device with the planes in HBM on the three grids of tools/clearance_cost.py -- 1174 x 160, 2936 x 400,
4096 x 4096 -- over three planes: a seeded 3-valued occupancy plane (-1 / 0 / 100 at 0.3 / 0.55 / 0.15) whose frontier
cells are the members, `full` (every cell a member: one region, one hot record) and `dots` (members at even ix and even
iy: the most regions a grid can hold, cut at max_regions).  For each, in the same process: the tile scheme at 8 and at 32
rows against LOM_REGIONS_OPT_TEST_NO_TILES (every adjacency through k_reg_merge), and on `full` the wave merge on against
off.  HIP events on the handle's stream around the call -- from its enqueue to the end of its read-back of the summary --
in --blocks alternating blocks, medians and ranges of the block values; the launches and waits of each from
lom_regions_stats.  Beside each, for context only and labelled as such: scipy.ndimage.label on the host over the same
members (one run, wall clock).  What bounds k_reg_merge and k_reg_accumulate is not stated: that needs counters, collected
in a run of their own.
    python tools/regions_cost.py [--blocks 5] [--no-scipy] > profiles/regions_cost.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25), (2936, 400, 0.1), (4096, 4096, 0.25)]  # width, height, r


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "note": "ms per call, HIP events on the handle's stream, the summary's read-back included; the planes in HBM",
           "bound_of_k_reg_merge": "NOT MEASURED (no counter run): likely atomics on few addresses",
           "bound_of_k_reg_accumulate": "NOT MEASURED (no counter run): likely atomics on few addresses",
           "runs": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    frontier = (capi.REGIONS_FRONTIER, 0, 0, 99, 1, capi.REGIONS_RANK_LABEL, 0)
    lethal = (capi.REGIONS_BYTES, 100, 100, 99, 1, capi.REGIONS_RANK_LABEL, 0)
    for width, height, res in GRIDS:
        rng = np.random.default_rng(width)
        u = rng.random((height, width))
        dots = np.zeros((height, width), np.int8)
        dots[0::2, 0::2] = 100
        planes = {"frontier": (np.where(u < 0.3, -1, np.where(u < 0.85, 0, 100)).astype(np.int8), frontier),
                  "full": (np.full((height, width), 100, np.int8), lethal), "dots": (dots, lethal)}
        dev = lom.RegionGrid(res, (0.0, 0.0), width, height)
        stream = torch.cuda.ExternalStream(L.lom_regions_stream(dev.handle))
        for name, (plane, params) in planes.items():
            d_plane = torch.from_numpy(plane).to("cuda:0")
            torch.cuda.synchronize()
            seen = {}

            def extract(rows, no_tiles, no_merge, key):
                dev.setOption(capi.REGIONS_OPT_TEST_TILE_ROWS, rows)
                dev.setOption(capi.REGIONS_OPT_TEST_NO_TILES, no_tiles)
                dev.setOption(capi.REGIONS_OPT_TEST_NO_WAVE_MERGE, no_merge)
                ms = timed(stream, lambda: seen.__setitem__(key, dev.extract(d_plane.data_ptr(), params, device=True)))
                seen[key + "_stats"] = dev.stats()
                return ms

            kinds = {"tiles_32_ms": lambda: extract(32, 0, 0, "t32"), "tiles_8_ms": lambda: extract(8, 0, 0, "t8"),
                     "no_tiles_ms": lambda: extract(32, 1, 0, "none")}
            if name == "full":
                kinds["tiles_32_no_wave_merge_ms"] = lambda: extract(32, 0, 1, "nomerge")
            names = list(kinds)
            labels = {}
            for k, fn in kinds.items():
                fn()  # warm-up: code objects, buffers
                labels[k] = dev.labels()
            per_block = {k: [] for k in names}
            for b in range(args.blocks):
                for k in (names if b % 2 == 0 else names[::-1]):
                    per_block[k].append(kinds[k]())
            rec = {"width": width, "height": height, "plane": name, "summary": seen["t32"],
                   "stats": {k: seen[k + "_stats"] for k in ("t32", "t8", "none")},
                   "same_bytes": bool(all(v.tobytes() == labels["tiles_32_ms"].tobytes() for v in labels.values()) and
                                      all(seen[k] == seen["t32"] for k in ("t8", "none")))}
            rec.update({k: _spread(v) for k, v in per_block.items()})
            med = {k: statistics.median(v) for k, v in per_block.items()}
            rec["tiles_32_over_no_tiles"] = round(med["tiles_32_ms"] / med["no_tiles_ms"], 4)
            rec["tiles_8_over_tiles_32"] = round(med["tiles_8_ms"] / med["tiles_32_ms"], 4)
            if name == "full":
                rec["wave_merge_over_none"] = round(med["tiles_32_ms"] / med["tiles_32_no_wave_merge_ms"], 4)
            if not args.no_scipy:
                from scipy import ndimage

                members = labels["tiles_32_ms"] != capi.REGIONS_NONE
                t0 = time.perf_counter()
                _, count = ndimage.label(members, structure=np.ones((3, 3), int))
                rec["context_scipy_label_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec["context_scipy_agrees"] = bool(count == seen["t32"]["regions"])
            out["runs"].append(rec)
            print("%d x %d %s: tiles 32 %.3f ms, tiles 8 %.3f ms, no tiles %.3f ms" % (width, height, name, med["tiles_32_ms"],
                  med["tiles_8_ms"], med["no_tiles_ms"]), file=sys.stderr, flush=True)
            dev.setOption(capi.REGIONS_OPT_TEST_TILE_ROWS, 0)
            dev.setOption(capi.REGIONS_OPT_TEST_NO_TILES, 0)
            dev.setOption(capi.REGIONS_OPT_TEST_NO_WAVE_MERGE, 0)
        del dev
    print(json.dumps(out))


if __name__ == "__main__":
    main()
