#!/usr/bin/env python3
"""What the visibility grid costs: one JSON line.
lom_visibility_cast_device with the plane in HBM on two grids of tools/regions_cost.py -- 1174 x 160 and 4096 x 4096 -- over
two seeded planes: `frontier` (-1 / 0 / 100 at 0.3 / 0.55 / 0.15: short rays, most end on a hit within a few cells) and
`open` (free ground with 1 % obstacles whose right half is unknown: long rays, most run to the range limit), from K = 64,
1024 and 16384 viewpoints on free cells, at (R, B) = (40, 256) and (120, 1024), under LOM_VIS_KEEP_WINDOWS.  For each, in
the same process: the default (the seen bits in an LDS window, four waves per workgroup) against LOM_VIS_OPT_TEST_NO_LDS
(the seen bits straight to the window in HBM) and against one wave per workgroup; then lom_visibility_select with n = 16
over the windows the default left.  HIP events on the handle's stream around the call -- from its enqueue to the end of
its read-back -- in --blocks alternating blocks, medians and ranges of the block values; the launches and waits of each
from lom_visibility_stats.  What bounds k_vis_cast is not stated: that needs counters, collected in a run of their own.
    python tools/visibility_cost.py [--blocks 5] > profiles/visibility_cost.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25), (4096, 4096, 0.25)]  # width, height, r
VIEWPOINTS = [64, 1024, 16384]
RANGE_BEAMS = [(40, 256), (120, 1024)]


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "note": "ms per call, HIP events on the handle's stream, the read-back of the summary (of the picks) included; the "
                   "plane in HBM, the viewpoints in host memory",
           "bound_of_k_vis_cast": "NOT MEASURED (no counter run): divergence between short and long rays, LDS atomics or the "
                                  "plane's loads",
           "runs": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for width, height, res in GRIDS:
        rng = np.random.default_rng(width)
        u = rng.random((height, width))
        open_plane = np.where(u < 0.01, 100, 0).astype(np.int8)
        open_plane[:, width // 2:][open_plane[:, width // 2:] == 0] = -1
        planes = {"frontier": np.where(u < 0.3, -1, np.where(u < 0.85, 0, 100)).astype(np.int8), "open": open_plane}
        dev = lom.VisibilityGrid(res, (0.0, 0.0), width, height)
        stream = torch.cuda.ExternalStream(L.lom_visibility_stream(dev.handle))
        for name, plane in planes.items():
            d_plane = torch.from_numpy(plane).to("cuda:0")
            torch.cuda.synchronize()
            free = np.argwhere(plane == 0)[:, ::-1]
            for k in VIEWPOINTS:
                vp = np.ascontiguousarray(free[rng.integers(0, len(free), k)], np.int32)
                for rng_cells, beams in RANGE_BEAMS:
                    params = (beams, rng_cells, 100, 0, capi.VIS_KEEP_WINDOWS)
                    seen = {}

                    def cast(no_lds, waves, key):
                        dev.setOption(capi.VIS_OPT_TEST_NO_LDS, no_lds)
                        dev.setOption(capi.VIS_OPT_TEST_WAVES, waves)
                        ms = timed(stream, lambda: seen.__setitem__(key, dev.cast(d_plane.data_ptr(), vp, params, device=True)))
                        seen[key + "_stats"] = dev.stats()
                        return ms

                    kinds = {"lds_4_waves_ms": lambda: cast(0, 4, "lds4"), "no_lds_4_waves_ms": lambda: cast(1, 4, "hbm4"),
                             "lds_1_wave_ms": lambda: cast(0, 1, "lds1")}
                    names = list(kinds)
                    records = {}
                    for kind, fn in kinds.items():
                        fn()  # warm-up: code objects, buffers
                        records[kind] = dev.records()
                    per_block = {kind: [] for kind in names}
                    for b in range(args.blocks):
                        for kind in (names if b % 2 == 0 else names[::-1]):
                            per_block[kind].append(kinds[kind]())
                    # the selection over the windows of a default cast
                    cast(0, 4, "lds4")
                    picks = []
                    select_ms = [timed(stream, lambda: picks.append(dev.select((16, 1, 0, 1)))) for _ in range(args.blocks + 1)][1:]
                    r = records["lds_4_waves_ms"]
                    rec = {"width": width, "height": height, "plane": name, "viewpoints": k, "range_cells": rng_cells, "beams": beams,
                           "summary": seen["lds4"], "mean_seen": round(float(r["seen"].mean()), 1), "mean_hits": round(float(r["hits"].mean()), 1),
                           "stats": {key: seen[key + "_stats"] for key in ("lds4", "hbm4", "lds1")}, "select_stats": dev.stats(),
                           "select_n": 16, "select_picked": len(picks[-1]), "select_ms": _spread(select_ms),
                           "same_bytes": bool(all(v.tobytes() == r.tobytes() for v in records.values()) and
                                              all(seen[key] == seen["lds4"] for key in ("hbm4", "lds1")) and
                                              all(v.tobytes() == picks[0].tobytes() for v in picks))}
                    rec.update({kind: _spread(v) for kind, v in per_block.items()})
                    med = {kind: statistics.median(v) for kind, v in per_block.items()}
                    rec["lds_over_no_lds"] = round(med["lds_4_waves_ms"] / med["no_lds_4_waves_ms"], 4)
                    rec["waves_4_over_1"] = round(med["lds_4_waves_ms"] / med["lds_1_wave_ms"], 4)
                    out["runs"].append(rec)
                    print("%d x %d %s K %d R %d B %d: lds %.3f ms, no lds %.3f ms, one wave %.3f ms, select %.3f ms" %
                          (width, height, name, k, rng_cells, beams, med["lds_4_waves_ms"], med["no_lds_4_waves_ms"], med["lds_1_wave_ms"],
                           statistics.median(select_ms)), file=sys.stderr, flush=True)
                    dev.setOption(capi.VIS_OPT_TEST_NO_LDS, 0)
                    dev.setOption(capi.VIS_OPT_TEST_WAVES, 0)
        del dev
    print(json.dumps(out))


if __name__ == "__main__":
    main()
