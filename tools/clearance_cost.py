#!/usr/bin/env python3
"""What the clearance grid costs: one JSON line.
Full updates (lom_clearance_update_device, planes in HBM) of three grids -- 1174 x 160 at R = 8 (the K = 512 grid of
tools/elevation_cost.py at 0.25 m with 2 m inflation), 2936 x 400 at R = 20, 4096 x 4096 at R = 40 -- each at 2 % and at
0.01 % obstacles (sparse maps are where the pruning of the column pass stops late), with the pruning on and off
(LOM_CLEAR_OPT_TEST_NO_PRUNE).  HIP events on the handle's stream around the call -- from its enqueue to the end of its
read-back of the summary -- in --blocks alternating blocks, medians and ranges of the block values.  Then a 256 x 256
windowed update in the middle of the largest grid and lom_clearance_query of 10^4 points (host arrays in and out).
Beside each full update, for context only and labelled as such: the same distance through
scipy.ndimage.distance_transform_edt on the host (one run, wall clock; it is not truncated at R), and the time the
bytes-per-cell floor -- 2 in, 3 out -- takes at the HBM peak.  What bounds k_clear_distance is not stated: that needs
counters, collected in a run of their own.
    python tools/clearance_cost.py [--blocks 5] [--no-scipy] > profiles/clearance_cost.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12  # the data sheet's figure for an MI355X
GRIDS = [(1174, 160, 0.25, 2.0, 8), (2936, 400, 0.1, 2.05, 20), (4096, 4096, 0.25, 10.0, 40)]  # width, height, r, inflation, R


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
           "note": "ms per call, HIP events on the handle's stream, the summary's read-back included; planes in HBM",
           "bound_of_k_clear_distance": "NOT MEASURED (no counter run)", "runs": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    rng = np.random.default_rng(1)
    for width, height, res, inflation, R in GRIDS:
        g = lom.ClearanceGrid(res, (0.0, 0.0), width, height)
        stream = torch.cuda.ExternalStream(L.lom_clearance_stream(g.handle))
        p = dict(inflation_radius=inflation, inscribed_radius=0.5, decay=1.5, flags=0)
        assert len(lom.clearanceCostTable(p, res)) == R * R + 1
        for share in (0.02, 0.0001):
            ob = rng.random((height, width)) < share
            occ = np.where(ob, 100, 0).astype(np.int8)
            elev = rng.integers(-1, 100, (height, width)).astype(np.int8)
            t_occ, t_elev = torch.from_numpy(occ).to("cuda:0"), torch.from_numpy(elev).to("cuda:0")
            torch.cuda.synchronize()
            seen = {}

            def full(no_prune):
                g.setOption(capi.CLEAR_OPT_TEST_NO_PRUNE, no_prune)
                return timed(stream, lambda: seen.__setitem__("summary", g.update(t_occ.data_ptr(), t_elev.data_ptr(), p, device=True)))

            kinds = {"prune_ms": lambda: full(0), "no_prune_ms": lambda: full(1)}
            names = list(kinds)
            for fn in kinds.values():
                fn()  # warm-up: the table, code objects
            per_block = {k: [] for k in names}
            for b in range(args.blocks):
                for k in (names if b % 2 == 0 else names[::-1]):
                    per_block[k].append(kinds[k]())
            cells = width * height
            rec = {"width": width, "height": height, "resolution": res, "R": R, "obstacle_share": share, "obstacles": int(ob.sum()),
                   "summary": seen["summary"]}
            rec.update({k: _spread(v) for k, v in per_block.items()})
            rec["cells_per_us"] = {k: round(cells / (1e3 * statistics.median(v)), 1) for k, v in per_block.items()}
            rec["context_hbm_floor_ms"] = round(5.0 * cells / HBM_PEAK_BYTES_PER_S * 1e3, 5)
            if not args.no_scipy:
                from scipy import ndimage

                t0 = time.perf_counter()
                ndimage.distance_transform_edt(~ob)
                rec["context_scipy_edt_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            out["runs"].append(rec)
        if (width, height) == (4096, 4096):
            g.setOption(capi.CLEAR_OPT_TEST_NO_PRUNE, 0)
            win = (width // 2 - 128, height // 2 - 128, 256, 256)
            windowed = lambda: timed(stream, lambda: g.update(t_occ.data_ptr(), t_elev.data_ptr(), p, window=win, device=True))
            windowed()
            out["window_256x256_ms"] = dict(_spread([windowed() for _ in range(2 * args.blocks)]), R=R, obstacle_share=share)
            xy = rng.uniform(-5.0, width * res + 5.0, (10000, 2)).astype(np.float32)
            query = lambda: timed(stream, lambda: g.query(xy))
            query()
            out["query_10000_points_ms"] = _spread([query() for _ in range(2 * args.blocks)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
