#!/usr/bin/env python3
"""What the navigation field costs: one JSON line.
lom_navfield_solve_device over the cost plane a ClearanceGrid left in HBM, on the three grids of tools/clearance_cost.py
-- 1174 x 160, 2936 x 400, 4096 x 4096 -- each at 2 % and at 0.01 % obstacles (inflated with an inscribed radius of one
cell, so that the dense planes stay navigable), with one goal in a corner and one in the middle.  For each, in the same process: the default (tiles of 32 x 32 relaxed in LDS until they settle, only marked tiles
active) against LOM_NAV_OPT_TEST_INNER_CAP = 1 with LOM_NAV_OPT_TEST_ALL_TILES = 1, which is the plain global sweep, one
per launch.  HIP events on the handle's stream around the call -- from its enqueue to the end of its read-back of the
summary -- in --blocks alternating blocks, medians and ranges of the block values; the launches and waits of each from
lom_navfield_stats.  Then lom_navfield_paths at K = 1 and K = 10^4 on the largest grid (cap 1024 cells; host arrays in and
out).  Beside the two smaller grids, for context only and labelled as such: scipy's Dijkstra on the host over the same
graph (one run, wall clock, the graph's construction not counted).  What bounds k_nav_relax -- launch latency along the
wavefront's path or the LDS sweeps -- is not stated: that needs counters, collected in a run of their own.
    python tools/navfield_cost.py [--blocks 5] [--no-scipy] [--no-sweep-on-largest] > profiles/navfield_cost.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25, 2.0), (2936, 400, 0.1, 2.05), (4096, 4096, 0.25, 10.0)]  # width, height, r, inflation
PARAMS = (50, 3, 400, 98, 0)  # neutral, factor, unknown_cost, max_passable, flags
STEPS = ((1, 0, 5), (0, 1, 5), (-1, 0, 5), (0, -1, 5), (1, 1, 7), (-1, 1, 7), (-1, -1, 7), (1, -1, 7))


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "n": len(xs)}


def scipy_dijkstra_ms(np, cost, goal):
    """the same field on the host: (ms of scipy.sparse.csgraph.dijkstra alone, the field as float64)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    h, w = cost.shape
    table = np.zeros(256, np.int64)
    table[:PARAMS[3] + 1] = PARAMS[0] + PARAMS[1] * np.arange(PARAMS[3] + 1)
    c = table[cost.view(np.uint8)]
    ok = c > 0
    idx = np.arange(h * w).reshape(h, w)
    rows, cols, vals = [], [], []

    def cut(a, dx, dy):  # the cells that have a neighbour at (dx, dy), and those neighbours
        ys = slice(max(0, -dy), h - max(0, dy))
        xs = slice(max(0, -dx), w - max(0, dx))
        yb = slice(max(0, dy), h - max(0, -dy))
        xb = slice(max(0, dx), w - max(0, -dx))
        return a[ys, xs], a[yb, xb], a[ys, xb], a[yb, xs]

    for dx, dy, ln in STEPS:
        oa, ob, oside1, oside2 = cut(ok, dx, dy)
        ia, ib, _, _ = cut(idx, dx, dy)
        ca = cut(c, dx, dy)[0]
        allowed = oa & ob & ((oside1 & oside2) if dx and dy else True)
        rows.append(ib[allowed]), cols.append(ia[allowed]), vals.append((ln * ca[allowed]).astype(np.float64))  # reversed: b -> a
    m = csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(h * w, h * w))
    t0 = time.perf_counter()
    d = dijkstra(m, directed=True, indices=[goal[1] * w + goal[0]], min_only=True)
    return round((time.perf_counter() - t0) * 1e3, 1), d.reshape(h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-sweep-on-largest", action="store_true", help="skip the plain global sweep on the 4096 x 4096 grid")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "note": "ms per call, HIP events on the handle's stream, the summary's read-back included; the cost plane in HBM",
           "params": dict(zip(("neutral", "factor", "unknown_cost", "max_passable", "flags"), PARAMS)),
           "bound_of_k_nav_relax": "NOT MEASURED (no counter run): launch latency along the wavefront's path, or the LDS sweeps",
           "runs": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    rng = np.random.default_rng(1)
    for width, height, res, inflation in GRIDS:
        clear = lom.ClearanceGrid(res, (0.0, 0.0), width, height)
        nav = lom.NavField(res, (0.0, 0.0), width, height)
        stream = torch.cuda.ExternalStream(L.lom_navfield_stream(nav.handle))
        # inscribed: one cell, so that at 2 % obstacles the plane stays navigable (an obstacle blocks itself and its 4 neighbours)
        cp = dict(inflation_radius=inflation, inscribed_radius=res, decay=1.5, flags=0)
        largest = (width, height) == (4096, 4096)
        for share in (0.02, 0.0001):
            ob = rng.random((height, width)) < share
            occ = np.where(ob, 100, 0).astype(np.int8)
            occ[0, 0] = occ[height // 2, width // 2] = 0
            clear.update(occ, None, cp)
            cost = clear.cost()[0]
            d_cost = C.c_void_p()
            assert L.lom_clearance_cost_device(clear.handle, C.byref(d_cost)) == 0
            for goal_name, goal in (("corner", (0, 0)), ("middle", (width // 2, height // 2))):
                # the nearest passable cell along the diagonal, should the inflation have taken the goal
                while (cost[goal[1], goal[0]] < 0 or cost[goal[1], goal[0]] > PARAMS[3]) and max(goal[0] + 2 - width, goal[1] + 2 - height) < 0:
                    goal = (goal[0] + 1, goal[1] + 1)
                goals = np.array([goal], np.int32)
                seen = {}

                def solve(cap, every, key):
                    nav.setOption(capi.NAV_OPT_TEST_INNER_CAP, cap)
                    nav.setOption(capi.NAV_OPT_TEST_ALL_TILES, every)
                    ms = timed(stream, lambda: seen.__setitem__(key, nav.solve(d_cost.value, PARAMS, goals, device=True)))
                    seen[key + "_stats"] = nav.stats()
                    return ms

                kinds = {"tiles_ms": lambda: solve(0, 0, "tiles")}
                if not (largest and args.no_sweep_on_largest):
                    kinds["global_sweep_ms"] = lambda: solve(1, 1, "sweep")
                names = list(kinds)
                fields = {}
                for k, fn in kinds.items():
                    fn()  # warm-up: code objects, buffers
                    fields[k] = nav.potential()
                per_block = {k: [] for k in names}
                for b in range(args.blocks):
                    for k in (names if b % 2 == 0 else names[::-1]):
                        per_block[k].append(kinds[k]())
                rec = {"width": width, "height": height, "resolution": res, "obstacle_share": share, "obstacles": int(ob.sum()),
                       "goal": goal_name, "goal_cell": list(goal), "summary": seen["tiles"], "tiles_stats": seen["tiles_stats"]}
                if "global_sweep_ms" in kinds:
                    rec["global_sweep_stats"] = seen["sweep_stats"]
                    rec["same_bytes"] = bool(fields["tiles_ms"].tobytes() == fields["global_sweep_ms"].tobytes() and seen["tiles"] == seen["sweep"])
                    rec["tiles_over_global_sweep"] = round(statistics.median(per_block["tiles_ms"]) / statistics.median(per_block["global_sweep_ms"]), 4)
                else:
                    rec["global_sweep_ms"] = "NOT MEASURED (--no-sweep-on-largest)"
                rec.update({k: _spread(v) for k, v in per_block.items()})
                if not args.no_scipy and not largest and share == 0.02:
                    ms, d = scipy_dijkstra_ms(np, cost, goal)
                    rec["context_scipy_dijkstra_host_ms"] = ms
                    got = fields["tiles_ms"]
                    rec["context_scipy_agrees"] = bool(np.array_equal(got == capi.NAV_UNREACHED, np.isinf(d)) and
                                                       np.array_equal(got[got != capi.NAV_UNREACHED].astype(np.float64), d[~np.isinf(d)]))
                out["runs"].append(rec)
        if largest:
            nav.setOption(capi.NAV_OPT_TEST_INNER_CAP, 0)
            nav.setOption(capi.NAV_OPT_TEST_ALL_TILES, 0)
            nav.solve(d_cost.value, PARAMS, np.array([(0, 0)], np.int32), device=True)
            for k in (1, 10000):
                starts = np.stack([rng.integers(0, width, k), rng.integers(0, height, k)], axis=1).astype(np.int32)
                lengths = {}
                walk = lambda: timed(stream, lambda: lengths.__setitem__("l", nav.paths(starts, 1024)[1]))
                walk()
                out["paths_%d_starts_cap_1024_ms" % k] = dict(_spread([walk() for _ in range(args.blocks)]), obstacle_share=share,
                                                              longest=int(lengths["l"].max()), walked=int((lengths["l"] > 0).sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
