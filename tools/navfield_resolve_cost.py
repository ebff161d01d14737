#!/usr/bin/env python3
"""What a re-solve of the navigation field costs after a local change: one JSON line.
The cost planes of tools/navfield_cost.py -- 1174 x 160 and 4096 x 4096, each at 2 % and at 0.01 % obstacles, left in HBM by a
ClearanceGrid -- with one goal in the corner.  The change is a wall, a column of 64 lethal cells, put into a 64 x 64 window
and taken out again, at three places: (a) in the corner far from the goal, the robot's neighbourhood; (b) half way; (c) next
to the goal.  For each, in the same process and on the same handle, lom_navfield_resolve_device under the three forms of
LOM_NAV_OPT_TEST_RESOLVE_FORM: 0, raise then relax (the default); 1, the threshold form; 2, the full solve from the kept
goals, which is the yardstick.  HIP events on the handle's stream around the call -- from its enqueue to the end of its
read-back of the summary -- in --blocks alternating blocks, medians and ranges of the block values; the counts of each
from lom_navfield_resolve_stats.  The three forms' fields are compared as bytes, with the wall in and with it out.  What
bounds k_nav_raise is not stated: that needs counters, collected in a run of their own.
    python tools/navfield_resolve_cost.py [--blocks 5] > profiles/navfield_resolve_cost.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25, 2.0), (4096, 4096, 0.25, 10.0)]  # width, height, r, inflation
PARAMS = (50, 3, 400, 98, 0)  # neutral, factor, unknown_cost, max_passable, flags
SIDE = 64
FORMS = {0: "raise_relax", 1: "threshold", 2: "full_solve"}


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
           "note": "ms per call, HIP events on the handle's stream, the summary's read-back included; both planes in HBM; "
                   "form 2 (the full solve from the kept goals, same handle, same process) is the yardstick",
           "params": dict(zip(("neutral", "factor", "unknown_cost", "max_passable", "flags"), PARAMS)),
           "bound_of_k_nav_raise": "NOT MEASURED (no counter run)",
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
        cp = dict(inflation_radius=inflation, inscribed_radius=res, decay=1.5, flags=0)
        for share in (0.02, 0.0001):
            ob = rng.random((height, width)) < share
            occ = np.where(ob, 100, 0).astype(np.int8)
            occ[0, 0] = 0
            clear.update(occ, None, cp)
            cost = clear.cost()[0]
            goal = (0, 0)
            while (cost[goal[1], goal[0]] < 0 or cost[goal[1], goal[0]] > PARAMS[3]) and max(goal[0] + 2 - width, goal[1] + 2 - height) < 0:
                goal = (goal[0] + 1, goal[1] + 1)
            goals = np.array([goal], np.int32)
            d_base = torch.from_numpy(cost).to("cuda:0")
            places = {"a_far_corner": (width - SIDE - 8, height - SIDE - 8), "b_half_way": ((width - SIDE) // 2, (height - SIDE) // 2),
                      "c_next_to_the_goal": (0, 0)}
            for place, (x0, y0) in places.items():
                window = (x0, y0, SIDE, SIDE)
                walled = cost.copy()
                walled[y0:y0 + SIDE, x0 + SIDE // 2] = 100
                d_wall = torch.from_numpy(walled).to("cuda:0")
                torch.cuda.synchronize()
                for opt in (capi.NAV_OPT_TEST_INNER_CAP, capi.NAV_OPT_TEST_ALL_TILES, capi.NAV_OPT_TEST_BATCH):
                    nav.setOption(opt, 0)
                first = nav.solve(d_base.data_ptr(), PARAMS, goals, device=True)
                seen = {}

                def resolve(form, d_plane, key):
                    nav.setOption(capi.NAV_OPT_TEST_RESOLVE_FORM, form)
                    ms = timed(stream, lambda: seen.__setitem__((form, key), nav.resolve(d_plane.data_ptr(), window, device=True)))
                    seen[(form, key, "stats")] = nav.resolveStats()
                    return ms

                # warm-up, and the bytes of every form with the wall in and with it out
                fields = {}
                for form in FORMS:
                    resolve(form, d_wall, "in")
                    fields[(form, "in")] = nav.potential()
                    resolve(form, d_base, "out")
                    fields[(form, "out")] = nav.potential()
                same = all(fields[(f, k)].tobytes() == fields[(2, k)].tobytes() and seen[(f, k)] == seen[(2, k)] for f in FORMS for k in ("in", "out"))
                per_block = {(f, k): [] for f in FORMS for k in ("in", "out")}
                for b in range(args.blocks):
                    for form in (list(FORMS) if b % 2 == 0 else list(FORMS)[::-1]):
                        per_block[(form, "in")].append(resolve(form, d_wall, "in"))
                        per_block[(form, "out")].append(resolve(form, d_base, "out"))
                rec = {"width": width, "height": height, "obstacle_share": share, "goal_cell": list(goal), "place": place, "window": list(window),
                       "solve_summary": first, "same_bytes_and_summaries": bool(same),
                       "cells_reached_wall_in": seen[(2, "in")]["cells_reached"], "cells_reached_wall_out": seen[(2, "out")]["cells_reached"]}
                for k in ("in", "out"):
                    base = statistics.median(per_block[(2, k)])
                    for form, name in FORMS.items():
                        rec["wall_%s_%s_ms" % (k, name)] = _spread(per_block[(form, k)])
                        rec["wall_%s_%s_stats" % (k, name)] = seen[(form, k, "stats")]
                        if form != 2:
                            rec["wall_%s_%s_over_full_solve" % (k, name)] = round(statistics.median(per_block[(form, k)]) / base, 4)
                out["runs"].append(rec)
                del d_wall
    print(json.dumps(out))


if __name__ == "__main__":
    main()
