#!/usr/bin/env python3
"""What the navigation field set costs against N solves of one field: one JSON line.
Planes as tools/navfield_cost.py makes them (the cost plane a ClearanceGrid left in HBM, inflated with an inscribed radius
of one cell) at 1174 x 160 and 4096 x 4096, each at 2 % and at 0.01 % obstacles.  n_fields = 1, 4, 16, 64 with one goal
per field on free cells spread over the grid.  lom_navset_solve_device against n_fields calls of lom_navfield_solve_device
on one field in the same process, which is what a caller did before the set existed.  HIP events on the handle's stream
around the calls, in --blocks alternating blocks, medians and ranges of the block values; launches and waits on both sides;
the fields compared as bytes in every case.  Then, at 16 fields, lom_navset_gather of the 16 x 16 matrix at the goals and
lom_navset_nearest.  No ratio is asserted: every case is recorded, also where the set loses.
    python tools/navset_cost.py [--blocks 5] [--fields 1,4,16,64] > profiles/navset_cost.json
    python tools/navset_cost.py --trace      (one case for a kernel trace in a run of its own: 4096 x 4096, 2 %, 16 fields, the
                                              set once and the 16 single solves once; prints nothing but a line of stats)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25, 2.0), (4096, 4096, 0.25, 10.0)]  # width, height, r, inflation: tools/navfield_cost.py's first and last
PARAMS = (50, 3, 400, 98, 0)  # neutral, factor, unknown_cost, max_passable, flags


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def plane_of(lom, np, rng, clear, width, height, res, inflation, share):
    """tools/navfield_cost.py's generator: random obstacles, the corner and the middle free, inflated by a ClearanceGrid"""
    ob = rng.random((height, width)) < share
    occ = np.where(ob, 100, 0).astype(np.int8)
    occ[0, 0] = occ[height // 2, width // 2] = 0
    clear.update(occ, None, dict(inflation_radius=inflation, inscribed_radius=res, decay=1.5, flags=0))
    return clear.cost()[0], int(ob.sum())


def goals_of(np, cost, n):
    """one goal per field, spread over the grid (a stratum of x per field, y by the golden ratio), moved along the diagonal
    to the next passable cell"""
    h, w = cost.shape
    out = []
    for i in range(n):
        x, y = int((i + 0.5) / n * w), int(((i + 0.5) * 0.6180339887) % 1.0 * h)
        while (cost[y, x] < 0 or cost[y, x] > PARAMS[3]) and x + 1 < w and y + 1 < h:
            x, y = x + 1, y + 1
        out.append(np.array([(x, y)], np.int32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--fields", default="1,4,16,64")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    counts = [16] if args.trace else [int(v) for v in args.fields.split(",")]
    out = {"device": torch.cuda.get_device_name(0),
           "note": "ms per call (the set) and per n_fields calls (one field), HIP events on the handle's stream, the summaries' "
                   "read-back included; the cost plane in HBM; one goal per field",
           "params": dict(zip(("neutral", "factor", "unknown_cost", "max_passable", "flags"), PARAMS)), "blocks": args.blocks, "runs": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    rng = np.random.default_rng(1)
    for width, height, res, inflation in (GRIDS[1:] if args.trace else GRIDS):
        clear = lom.ClearanceGrid(res, (0.0, 0.0), width, height)
        nav = lom.NavField(res, (0.0, 0.0), width, height)
        nav_stream = torch.cuda.ExternalStream(L.lom_navfield_stream(nav.handle))
        for share in ((0.02,) if args.trace else (0.02, 0.0001)):
            cost, obstacles = plane_of(lom, np, rng, clear, width, height, res, inflation, share)
            d_cost = C.c_void_p()
            assert L.lom_clearance_cost_device(clear.handle, C.byref(d_cost)) == 0
            for n in counts:
                goals = goals_of(np, cost, n)
                navs = lom.NavFieldSet(res, (0.0, 0.0), width, height, n)
                set_stream = torch.cuda.ExternalStream(L.lom_navset_stream(navs.handle))
                seen = {}

                def solve_set():
                    seen["set"] = navs.solveDevice(d_cost.value, PARAMS, goals)
                    seen["set_stats"] = navs.stats()

                def solve_singles():
                    launches = waits = 0
                    seen["single"] = []
                    for g in goals:
                        seen["single"].append(nav.solve(d_cost.value, PARAMS, g, device=True))
                        st = nav.stats()
                        launches, waits = launches + st["launches"], waits + st["waits"]
                    seen["single_stats"] = dict(launches=launches, waits=waits, slowest_launches=0)

                if args.trace:
                    solve_set()
                    solve_singles()
                    print(json.dumps({"trace_case": [width, height, share, n], "set_stats": seen["set_stats"], "single_stats": seen["single_stats"]}))
                    return
                # warm-up, and the bytes: every field of the set against the single solve of its goal
                solve_set()
                same, slowest = seen["set"] is not None, 0
                for i, g in enumerate(goals):
                    sm = nav.solve(d_cost.value, PARAMS, g, device=True)
                    slowest = max(slowest, nav.stats()["launches"])
                    same = same and sm == seen["set"][i] and nav.potential().tobytes() == navs.potential(i).tobytes()
                kinds = {"set_ms": lambda: timed(set_stream, solve_set), "singles_ms": lambda: timed(nav_stream, solve_singles)}
                names = list(kinds)
                per_block = {k: [] for k in names}
                for b in range(args.blocks):
                    for k in (names if b % 2 == 0 else names[::-1]):
                        per_block[k].append(kinds[k]())
                seen["single_stats"]["slowest_launches"] = slowest
                rec = {"width": width, "height": height, "obstacle_share": share, "obstacles": obstacles, "n_fields": n,
                       "goal_cells": [g[0].tolist() for g in goals][:8], "same_bytes_and_summaries": bool(same),
                       "set_stats": seen["set_stats"], "single_stats": seen["single_stats"]}
                rec.update({k: _spread(v) for k, v in per_block.items()})
                rec["singles_over_set"] = round(statistics.median(per_block["singles_ms"]) / statistics.median(per_block["set_ms"]), 4)
                if n == 16:
                    at = np.concatenate(goals)
                    box = {}
                    navs.gather(at), navs.nearest()  # warm-up: buffers
                    rec["gather_16x16_ms"] = _spread([timed(set_stream, lambda: box.__setitem__("m", navs.gather(at))) for _ in range(args.blocks)])
                    rec["nearest_ms"] = _spread([timed(set_stream, lambda: box.__setitem__("n", navs.nearest())) for _ in range(args.blocks)])
                    rec["matrix_diagonal_zero"] = bool((np.diag(box["m"]) == 0).all())
                    rec["matrix_symmetric"] = bool((box["m"] == box["m"].T).all())
                    union = nav.solve(d_cost.value, PARAMS, at, device=True)
                    rec["nearest_potential_is_the_union_solve"] = bool(box["n"][1].tobytes() == nav.potential().tobytes())
                    rec["cells_owned_sum_is_cells_reached"] = bool(int(box["n"][2].sum()) == union["cells_reached"])
                out["runs"].append(rec)
                del navs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
