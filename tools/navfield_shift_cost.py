#!/usr/bin/env python3
"""What it costs to keep a navigation field through a shift: one JSON line.
A world cost plane a little larger than the grid -- 1174 x 160 and 4096 x 4096, each at 2 % and at 0.01 % obstacles, left by a
ClearanceGrid of the world's size -- of which the grid sees a window; the window moves by (32, 0), (0, 32), (33, 17) and (1, 1)
cells.  One goal, at three places: far ahead on the leading side, far behind on the trailing side (it stays in the grid), and
in the corner that leaves.  Compared, in the same process and on a pair of handles that hold the same solved state:
  keep:   lom_navfield_shift_resolve_device (forms 0, the default, and 2, the full relaxation from the moved goals)
  today:  lom_navfield_shift, then lom_navfield_solve_device with the goals passed again
HIP events on each handle's stream around the calls -- from the first enqueue to the end of the read-back of the summary -- in
--blocks alternating blocks, medians and ranges of the block values; the state before the shift is put back by a full solve
outside the timed region.  The fields of both sides are compared as bytes.  The mover alone: a device-to-device
hipMemcpyAsync of 5 bytes per cell on the same stream is timed here; k_nav_shift_diff's own duration comes from
    rocprofv3 --kernel-trace --output-format csv -d out -o kt -- python tools/navfield_shift_cost.py --trace
(--trace: nothing is timed, three shift-resolves per grid and shift).
    python tools/navfield_shift_cost.py [--blocks 5] > profiles/navfield_shift_cost.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25, 2.0), (4096, 4096, 0.25, 10.0)]  # width, height, r, inflation
SHIFTS = [(32, 0), (0, 32), (33, 17), (1, 1)]
MARGIN = 40                                                  # the world is this much larger than the grid on both axes
PARAMS = (50, 3, 400, 98, 0)  # neutral, factor, unknown_cost, max_passable, flags


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits),
            "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "note": "ms per call, HIP events on the handle's stream, the summary's read-back included; all planes in HBM; 'today' is "
                   "lom_navfield_shift + lom_navfield_solve_device with the goals passed again",
           "params": dict(zip(("neutral", "factor", "unknown_cost", "max_passable", "flags"), PARAMS)),
           "runs": [], "mover": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def passable_near(cost, x, y):
        h, w = cost.shape
        for r in range(0, 64):
            for yy in range(max(0, y - r), min(h, y + r + 1)):
                for xx in range(max(0, x - r), min(w, x + r + 1)):
                    if 0 <= cost[yy, xx] <= PARAMS[3]:
                        return xx, yy
        raise SystemExit("no passable cell near (%d, %d)" % (x, y))

    rng = np.random.default_rng(1)
    for width, height, res, inflation in GRIDS:
        ww, wh = width + MARGIN, height + MARGIN
        world_clear = lom.ClearanceGrid(res, (0.0, 0.0), ww, wh)
        cp = dict(inflation_radius=inflation, inscribed_radius=res, decay=1.5, flags=0)
        for share in (0.02, 0.0001):
            occ = np.where(rng.random((wh, ww)) < share, 100, 0).astype(np.int8)
            world_clear.update(occ, None, cp)
            world = world_clear.cost()[0]
            base = np.ascontiguousarray(world[:height, :width])
            d_base = torch.from_numpy(base).to("cuda:0")
            for dx, dy in SHIFTS:
                new = np.ascontiguousarray(world[dy:dy + height, dx:dx + width])
                d_new = torch.from_numpy(new).to("cuda:0")
                torch.cuda.synchronize()
                places = {"ahead_on_the_leading_side": (width - 8, height - 8), "behind_on_the_trailing_side": (dx + 8, dy + 8),
                          "in_the_corner_that_leaves": (0, 0)}
                for place, (gx, gy) in places.items():
                    if place == "in_the_corner_that_leaves":      # a cell whose new index is outside the grid
                        gx, gy = passable_near(base[:max(dy, 1), :] if dy else base[:, :max(dx, 1)], 0, 0)
                    else:
                        gx, gy = passable_near(base, gx, gy)
                    goals = np.array([(gx, gy)], np.int32)
                    moved_goals = np.array([(gx - dx, gy - dy)], np.int32)   # outside the grid for the goal that leaves: rejected
                    keep, today = lom.NavField(res, (0.0, 0.0), width, height), lom.NavField(res, (0.0, 0.0), width, height)
                    s_keep = torch.cuda.ExternalStream(L.lom_navfield_stream(keep.handle))
                    s_today = torch.cuda.ExternalStream(L.lom_navfield_stream(today.handle))
                    seen = {}

                    def put_back(nav):
                        nav.shift(-dx, -dy)                         # (dyadic resolution: the first origin, exactly)
                        return nav.solve(d_base.data_ptr(), PARAMS, goals, device=True)

                    def run_keep(form):
                        keep.setOption(capi.NAV_OPT_TEST_RESOLVE_FORM, form)
                        ms = timed(s_keep, lambda: seen.__setitem__(("keep", form), keep.shiftResolve(dx, dy, d_new.data_ptr(), None, device=True)))
                        seen[("keep", form, "stats")] = dict(keep.resolveStats(), **keep.shiftStats())
                        return ms

                    def run_today():
                        def both():
                            today.shift(dx, dy)
                            seen["today"] = today.solve(d_new.data_ptr(), PARAMS, moved_goals, device=True)
                        return timed(s_today, both)

                    first = keep.solve(d_base.data_ptr(), PARAMS, goals, device=True)
                    today.solve(d_base.data_ptr(), PARAMS, goals, device=True)
                    if args.trace:
                        for _ in range(3):
                            run_keep(0)
                            put_back(keep)
                        continue
                    # warm-up, and the bytes of both sides
                    fields = {}
                    for form in (0, 2):
                        run_keep(form)
                        fields[form] = keep.potential()
                        put_back(keep)
                    run_today()
                    fields["today"] = today.potential()
                    put_back(today)
                    same = all(fields[k].tobytes() == fields["today"].tobytes() for k in (0, 2))
                    same = same and all({k: v for k, v in seen[("keep", f)].items() if not k.startswith("goals_")} ==
                                        {k: v for k, v in seen["today"].items() if not k.startswith("goals_")} for f in (0, 2))
                    per_block = {"keep_raise_relax": [], "keep_full_relaxation": [], "today_shift_then_solve": []}
                    for b in range(args.blocks):
                        order = ["keep_raise_relax", "keep_full_relaxation", "today_shift_then_solve"]
                        for name in (order if b % 2 == 0 else order[::-1]):
                            if name == "today_shift_then_solve":
                                per_block[name].append(run_today())
                                put_back(today)
                            else:
                                per_block[name].append(run_keep(0 if name == "keep_raise_relax" else 2))
                                put_back(keep)
                    base_ms = statistics.median(per_block["today_shift_then_solve"])
                    rec = {"width": width, "height": height, "obstacle_share": share, "shift": [dx, dy], "goal": place, "goal_cell": [int(gx), int(gy)],
                           "solve_summary": first, "same_bytes_and_cell_counts": bool(same), "cells_reached_after": seen["today"]["cells_reached"],
                           "stats_raise_relax": seen[("keep", 0, "stats")], "stats_full_relaxation": seen[("keep", 2, "stats")]}
                    for name, xs in per_block.items():
                        rec[name + "_ms"] = _spread(xs)
                    for name in ("keep_raise_relax", "keep_full_relaxation"):
                        rec[name + "_over_today"] = round(statistics.median(per_block[name]) / base_ms, 4)
                    out["runs"].append(rec)
                    del keep, today
                del d_new
            # the yardstick of the mover: 5 bytes per cell, device to device, on a stream
            if not args.trace:
                n = width * height
                src, dst = torch.zeros(5 * n, dtype=torch.int8, device="cuda:0"), torch.empty(5 * n, dtype=torch.int8, device="cuda:0")
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    dst.copy_(src)
                    xs = [timed(s, lambda: dst.copy_(src)) for _ in range(args.blocks * 4)]
                out["mover"].append({"width": width, "height": height, "obstacle_share": share, "memcpy_d2d_5_bytes_per_cell_ms": _spread(xs),
                                     "k_nav_shift_diff_ms": "from the kernel trace (--trace): profiles/navfield_shift_kernels.txt"})
    if not args.trace:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
