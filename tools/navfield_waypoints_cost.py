#!/usr/bin/env python3
"""What the line-of-sight shortcuts of lom_navfield_waypoints cost: one JSON line.
The grids of tools/navfield_cost.py's path timing and its smallest one -- 4096 x 4096 and 1174 x 160 -- at 2 % and at 0.01 %
obstacles, once straight (the obstacle plane itself, max_cell_cost 0) and once behind a ClearanceGrid (its inflated cost,
max_cell_cost = neutral: shortcuts keep outside the inflation radius), one goal in the corner, K = 1 and K = 10^4 random
starts, route_cap 1024, lookahead W = 64 and W = 1024, wp_cap 64.  On one handle and the same starts, through the C ABI with
the host arrays made beforehand: lom_navfield_paths with cap = route_cap -- the trace and its copy-out of K x cap cells --
against lom_navfield_waypoints in its default form (a wave per route) and under LOM_NAV_OPT_TEST_SHORTCUT_SERIAL (a lane per
route) -- the same trace, the shortcut pass, and a copy-out of K x wp_cap cells.  HIP events on the handle's stream round
each call, --blocks alternating blocks, medians and ranges of the block values.  Beside each: the mean waypoints per walked
route and, over the first 200 routes, the mean number of candidates an anchor tests when they are taken one after another
from the farthest (the serial form's work; the wave form tests them 64 at a time).  The two forms' outputs are compared as
bytes.  What bounds k_nav_shortcut is not stated: that needs counters, collected in a run of their own.
    python tools/navfield_waypoints_cost.py [--blocks 5] > profiles/navfield_waypoints_cost.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25, 2.0), (4096, 4096, 0.25, 10.0)]  # width, height, r, inflation
PARAMS = (50, 3, 400, 98, 0)  # neutral, factor, unknown_cost, max_passable, flags
ROUTE_CAP, WP_CAP = 1024, 64


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "n": len(xs)}


def tested_per_anchor(route, wp, lookahead):
    """(anchors, candidates tested one after another from the farthest) from a route and its waypoints"""
    at, i = [], 0
    for c in wp:
        while route[i] != c:
            i += 1
        at.append(i)
    n, tested = len(route), 0
    for a, nxt in zip(at, at[1:]):
        hi = min(a + lookahead, n - 1)
        tested += hi - max(nxt, a + 2) + 1 if nxt > a + 1 else hi - a - 1
    return len(at) - 1, tested


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
           "note": "ms per call, HIP events on the handle's stream, host arrays made beforehand; paths copies out K x route_cap "
                   "cells, waypoints K x wp_cap; waypoints minus paths is the shortcut pass less the smaller copy",
           "params": dict(zip(("neutral", "factor", "unknown_cost", "max_passable", "flags"), PARAMS)),
           "route_cap": ROUTE_CAP, "wp_cap": WP_CAP, "bound_of_k_nav_shortcut": "NOT MEASURED (no counter run)", "runs": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = fn()
        e1.record(stream)
        e1.synchronize()
        assert rc == 0, rc
        return e0.elapsed_time(e1)

    rng = np.random.default_rng(1)
    for width, height, res, inflation in GRIDS:
        clear = lom.ClearanceGrid(res, (0.0, 0.0), width, height)
        nav = lom.NavField(res, (0.0, 0.0), width, height)
        stream = torch.cuda.ExternalStream(L.lom_navfield_stream(nav.handle))
        cp = dict(inflation_radius=inflation, inscribed_radius=res, decay=1.5, flags=0)
        for share in (0.02, 0.0001):
            occ = np.where(rng.random((height, width)) < share, 100, 0).astype(np.int8)
            occ[0, 0] = 0
            for mode in ("straight", "clearance"):
                if mode == "straight":
                    cost, mcc = occ, 0
                else:
                    clear.update(occ, None, cp)
                    cost, mcc = clear.cost()[0], PARAMS[0]
                goal = (0, 0)
                while (cost[goal[1], goal[0]] < 0 or cost[goal[1], goal[0]] > PARAMS[3]) and max(goal[0] + 2 - width, goal[1] + 2 - height) < 0:
                    goal = (goal[0] + 1, goal[1] + 1)
                summary = nav.solve(cost, PARAMS, np.array([goal], np.int32))
                for k in (1, 10000):
                    starts = np.stack([rng.integers(0, width, k), rng.integers(0, height, k)], axis=1).astype(np.int32)
                    if k == 1:
                        starts[0] = (width - 1, height - 1)  # the longest way
                    routes, lengths = np.zeros((k, ROUTE_CAP, 2), np.uint16), np.zeros(k, np.uint32)
                    cells, counts, lens = np.zeros((k, WP_CAP, 2), np.uint16), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
                    walk = lambda: L.lom_navfield_paths(nav.handle, 0, starts.ctypes.data, k, routes.ctypes.data, ROUTE_CAP, lengths.ctypes.data)
                    for lookahead in (64, 1024):
                        prm = capi.NavFieldWaypointParams(mcc, lookahead, ROUTE_CAP, 0)
                        cut = lambda: L.lom_navfield_waypoints(nav.handle, 0, starts.ctypes.data, k, C.byref(prm), cells.ctypes.data, WP_CAP,
                                                               counts.ctypes.data, lens.ctypes.data)
                        forms = {"paths": (None, walk), "waypoints": (0, cut), "waypoints_serial": (1, cut)}
                        kept = {}
                        for name, (serial, fn) in forms.items():  # warm-up, and the bytes of both forms
                            if serial is not None:
                                nav.setOption(capi.NAV_OPT_TEST_SHORTCUT_SERIAL, serial)
                            timed(stream, fn)
                            kept[name] = (cells.tobytes(), counts.tobytes(), lens.tobytes())
                        per_block = {name: [] for name in forms}
                        for b in range(args.blocks):
                            for name in (list(forms) if b % 2 == 0 else list(forms)[::-1]):
                                if forms[name][0] is not None:
                                    nav.setOption(capi.NAV_OPT_TEST_SHORTCUT_SERIAL, forms[name][0])
                                per_block[name].append(timed(stream, forms[name][1]))
                        nav.setOption(capi.NAV_OPT_TEST_SHORTCUT_SERIAL, 0)
                        assert cut() == 0
                        walked = counts > 0
                        anchors = tested = 0
                        for i in np.flatnonzero(walked & (counts <= WP_CAP))[:200]:
                            a, t = tested_per_anchor([tuple(c) for c in routes[i, :min(int(lengths[i]), ROUTE_CAP)].tolist()],
                                                     [tuple(c) for c in cells[i, :counts[i]].tolist()], lookahead)
                            anchors, tested = anchors + a, tested + t
                        med = {name: statistics.median(v) for name, v in per_block.items()}
                        rec = {"width": width, "height": height, "obstacle_share": share, "plane": mode, "max_cell_cost": mcc,
                               "cells_reached": summary["cells_reached"], "starts": k, "lookahead": lookahead, "walked": int(walked.sum()),
                               "longest_route": int(lengths.max()), "mean_route_cells": round(float(np.minimum(lengths[walked], ROUTE_CAP).mean()), 2) if walked.any() else 0,
                               "mean_waypoints": round(float(counts[walked].mean()), 2) if walked.any() else 0,
                               "mean_candidates_per_anchor_one_by_one": round(tested / anchors, 2) if anchors else 0,
                               "same_bytes_both_forms": kept["waypoints"] == kept["waypoints_serial"],
                               "shortcut_ms_waypoints_minus_paths": round(med["waypoints"] - med["paths"], 4),
                               "serial_over_default": round(med["waypoints_serial"] / med["waypoints"], 3)}
                        for name in forms:
                            rec[name + "_ms"] = _spread(per_block[name])
                        out["runs"].append(rec)
                        print("%d x %d, %g, %s, K = %d, W = %d: done" % (width, height, share, mode, k, lookahead), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
