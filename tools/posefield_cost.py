#!/usr/bin/env python3
"""What a pose field costs: one JSON document.
Planes as tools/navfield_cost.py makes them (the cost plane a ClearanceGrid left in HBM, inflated with an inscribed radius
of one cell) at 1174 x 160 and 4096 x 4096, each at 2 % and at 0.01 % obstacles; one goal, the passable cell nearest the
middle under h = -1; the footprints {(0, 0)} and a 9 x 3-cell rectangle at half-cell spacing; flags 0 and SPIN | REVERSE.
Per case lom_posefield_solve_device, the same call under the all-tiles switch (the plain global sweep), and -- as context
only: the pose field moves eight times the state -- lom_navfield_solve_device on the same plane and goal cell, all in the
same process.  HIP events on the handle's stream around the calls, in --blocks alternating blocks, medians and ranges of the
block values; launches and waits from lom_posefield_stats; the two pose solves compared as bytes.  Then a solve without
goals at F = 1, 77 and 1024 on the large grid: k_pose_layers, the fill, one batch of launches that find no tile and the
report, so the difference to F = 1 is the layers'.  No ratio is asserted: every case is recorded.
    python tools/posefield_cost.py [--blocks 5] [--out profiles/posefield_cost.json]
    python tools/posefield_cost.py --trace     (one case for a kernel trace in a run of its own: 4096 x 4096, 2 %, the 9 x 3
                                                rectangle, SPIN | REVERSE, once; prints a line of stats)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25, 2.0), (4096, 4096, 0.25, 10.0)]  # width, height, r, inflation: tools/navfield_cost.py's first and last
NAV = (50, 3, 400, 98, 0)  # neutral, factor, unknown_cost, max_passable, flags
TURN, SPIN_COST, REVERSE_COST = 20, 30, 200


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def plane_of(np, rng, clear, width, height, res, inflation, share):
    """tools/navfield_cost.py's generator: random obstacles, the corner and the middle free, inflated by a ClearanceGrid"""
    ob = rng.random((height, width)) < share
    occ = np.where(ob, 100, 0).astype(np.int8)
    occ[0, 0] = occ[height // 2, width // 2] = 0
    clear.update(occ, None, dict(inflation_radius=inflation, inscribed_radius=res, decay=1.5, flags=0))
    return clear.cost()[0], int(ob.sum())


def lattice(np, nx, ny, spacing):
    xs, ys = (np.arange(nx) - (nx - 1) / 2) * spacing, (np.arange(ny) - (ny - 1) / 2) * spacing
    return np.array([(int(x), int(y)) for x in xs for y in ys], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posefield_cost.json"))
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi

    L = capi.lib()
    torch.zeros(1, device="cuda:0")
    footprints = {"point": np.zeros((1, 2), np.int32), "9x3": lattice(np, 17, 5, 128)}
    flag_sets = {"0": 0, "SPIN|REVERSE": capi.POSE_SPIN | capi.POSE_REVERSE}
    out = {"device": torch.cuda.get_device_name(0),
           "note": "ms per call, HIP events on the handle's stream, the summary's read-back included; the cost plane in HBM; one goal",
           "nav": dict(zip(("neutral", "factor", "unknown_cost", "max_passable", "flags"), NAV)),
           "costs": dict(turn_cost=TURN, spin_cost=SPIN_COST, reverse_cost=REVERSE_COST), "blocks": args.blocks, "runs": [], "layers": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def save():
        if not args.trace:
            with open(args.out, "w") as f:
                f.write(json.dumps(out) + "\n")

    rng = np.random.default_rng(1)
    for width, height, res, inflation in (GRIDS[1:] if args.trace else GRIDS):
        clear = lom.ClearanceGrid(res, (0.0, 0.0), width, height)
        nav = lom.NavField(res, (0.0, 0.0), width, height)
        pose = lom.PoseField(res, (0.0, 0.0), width, height)
        nav_stream = torch.cuda.ExternalStream(L.lom_navfield_stream(nav.handle))
        pose_stream = torch.cuda.ExternalStream(L.lom_posefield_stream(pose.handle))
        for share in ((0.02,) if args.trace else (0.02, 0.0001)):
            cost, obstacles = plane_of(np, rng, clear, width, height, res, inflation, share)
            d_cost = C.c_void_p()
            assert L.lom_clearance_cost_device(clear.handle, C.byref(d_cost)) == 0
            for fp_name, fp in footprints.items():
                for flag_name, flags in flag_sets.items():
                    if args.trace and (fp_name, flag_name) != ("9x3", "SPIN|REVERSE"):
                        continue
                    params = (NAV, TURN, SPIN_COST, REVERSE_COST, flags)
                    # the goal: the cell nearest the middle that some heading of this footprint fits
                    pose.solve(d_cost.value, params, fp, np.zeros((0, 3), np.int32), device=True)
                    fits = np.argwhere(pose.layers().any(axis=0))
                    gy, gx = fits[np.argmin(np.abs(fits - (height // 2, width // 2)).sum(axis=1))]
                    goal = np.array([(gx, gy, -1)], np.int32)
                    seen = {}

                    def solve(every):
                        pose.setOption(capi.POSE_OPT_TEST_ALL_TILES, every)
                        seen["summary", every] = pose.solve(d_cost.value, params, fp, goal, device=True)
                        seen["stats", every] = pose.stats()

                    def solve_nav():
                        seen["nav"] = nav.solve(d_cost.value, NAV, goal[:, :2], device=True)
                        seen["nav_stats"] = nav.stats()

                    if args.trace:
                        solve(0)
                        print(json.dumps({"trace_case": [width, height, share, fp_name, flag_name], "stats": seen["stats", 0],
                                          "summary": seen["summary", 0]}))
                        return
                    solve(1)
                    swept = pose.potential().tobytes()
                    solve(0)
                    same = pose.potential().tobytes() == swept and seen["summary", 0] == seen["summary", 1]
                    kinds = {"marks_ms": lambda: timed(pose_stream, lambda: solve(0)), "all_tiles_ms": lambda: timed(pose_stream, lambda: solve(1)),
                             "navfield_ms": lambda: timed(nav_stream, solve_nav)}
                    names = list(kinds)
                    per_block = {k: [] for k in names}
                    for b in range(args.blocks):
                        for k in (names if b % 2 == 0 else names[::-1]):
                            per_block[k].append(kinds[k]())
                    pose.setOption(capi.POSE_OPT_TEST_ALL_TILES, 0)
                    sm = seen["summary", 0]
                    rec = {"width": width, "height": height, "obstacle_share": share, "obstacles": obstacles, "footprint": fp_name,
                           "samples": len(fp), "flags": flag_name, "goal": goal[0].tolist(), "same_bytes_and_summaries": bool(same),
                           "summary": sm, "reached_share_of_passable": round(sm["states_reached"] / max(sm["states_reached"] + sm["states_unreached"], 1), 4),
                           "marks_stats": seen["stats", 0], "all_tiles_stats": seen["stats", 1], "navfield_stats": seen["nav_stats"]}
                    rec.update({k: _spread(v) for k, v in per_block.items()})
                    rec["all_tiles_over_marks"] = round(statistics.median(per_block["all_tiles_ms"]) / statistics.median(per_block["marks_ms"]), 4)
                    out["runs"].append(rec)
                    save()
            if (width, height) == GRIDS[-1][:2] and share == 0.02:
                for name, fp in (("F=1", footprints["point"]), ("F=77", lattice(np, 11, 7, 128)), ("F=1024", lattice(np, 32, 32, 64))):
                    params = (NAV, TURN, SPIN_COST, REVERSE_COST, 0)
                    run = lambda: pose.solve(d_cost.value, params, fp, np.zeros((0, 3), np.int32), device=True)
                    run()
                    cells = [len(s) for s in lom.posefieldStencils(fp)]
                    out["layers"].append({"width": width, "height": height, "footprint": name, "stencil_cells": cells,
                                          "solve_without_goals_ms": _spread([timed(pose_stream, run) for _ in range(args.blocks)])})
                    save()
        del pose, nav, clear
    save()
    print(json.dumps({"written": args.out, "runs": len(out["runs"])}))


if __name__ == "__main__":
    main()
