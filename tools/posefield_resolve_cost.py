#!/usr/bin/env python3
"""What a pose field's re-solve costs against the full solve on the same handle: one JSON document.
Planes as tools/posefield_cost.py makes them, at 1174 x 160 and 4096 x 4096, each at 2 % and at 0.01 % obstacles; one goal
under h = -1, the cell nearest (24, 24) that the footprint fits; the footprints {(0, 0)} and a 9 x 3-cell rectangle; flags 0
and SPIN | REVERSE.  The change is the navigation field's re-solve case: a wall of 64 cells put into, then taken out of, a
64 x 64 window, both planes in HBM -- the window in the far corner from the goal (the robot's neighbourhood), half way, and
next to the goal.  Per case lom_posefield_resolve_device under the default form (raise, then relax) and under
LOM_POSE_OPT_TEST_RESOLVE_FORM 1 (the layers over the whole plane and the full relaxation) on the same handle in the same
process, and -- as context only -- lom_posefield_solve_device of the walled plane on a second handle with the goal passed
again.  HIP events on the handle's stream around the calls, in --blocks alternating blocks, medians and ranges of the block
values; the counters from lom_posefield_resolve_stats; the two forms compared as bytes (P and the floor).  No ratio is
asserted: every case is recorded.
    python tools/posefield_resolve_cost.py [--blocks 5] [--out profiles/posefield_resolve_cost.json] [--small]
    python tools/posefield_resolve_cost.py --trace   (one case for a kernel trace in a run of its own: 4096 x 4096, 2 %, the
                                                      9 x 3 rectangle, SPIN | REVERSE, the far corner, wall in and out once)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160, 0.25, 2.0), (4096, 4096, 0.25, 10.0)]  # width, height, r, inflation: tools/posefield_cost.py's
NAV = (50, 3, 400, 98, 0)  # neutral, factor, unknown_cost, max_passable, flags
TURN, SPIN_COST, REVERSE_COST = 20, 30, 200
WINDOW = 64


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def plane_of(np, rng, clear, width, height, res, inflation, share):
    """tools/posefield_cost.py's generator: random obstacles inflated by a ClearanceGrid; the goal's and the windows'
    neighbourhoods are left to the obstacles as they fall"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posefield_resolve_cost.json"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--small", action="store_true", help="the small grid only")
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
           "note": "ms per call, HIP events on the handle's stream, the read-backs included; both planes in HBM; one goal; "
                   "form0: raise, then relax; form1: the full solve on the same handle; solve: lom_posefield_solve_device on a second handle",
           "nav": dict(zip(("neutral", "factor", "unknown_cost", "max_passable", "flags"), NAV)),
           "costs": dict(turn_cost=TURN, spin_cost=SPIN_COST, reverse_cost=REVERSE_COST), "blocks": args.blocks, "runs": []}

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
    grids = GRIDS[1:] if args.trace else GRIDS[:1] if args.small else GRIDS
    for width, height, res, inflation in grids:
        clear = lom.ClearanceGrid(res, (0.0, 0.0), width, height)
        pose, second = lom.PoseField(res, (0.0, 0.0), width, height), lom.PoseField(res, (0.0, 0.0), width, height)
        pose_stream = torch.cuda.ExternalStream(L.lom_posefield_stream(pose.handle))
        second_stream = torch.cuda.ExternalStream(L.lom_posefield_stream(second.handle))
        for share in ((0.02,) if args.trace else (0.02, 0.0001)):
            cost, obstacles = plane_of(np, rng, clear, width, height, res, inflation, share)
            t_base = torch.from_numpy(cost).to("cuda:0")
            for fp_name, fp in footprints.items():
                for flag_name, flags in flag_sets.items():
                    if args.trace and (fp_name, flag_name) != ("9x3", "SPIN|REVERSE"):
                        continue
                    params = (NAV, TURN, SPIN_COST, REVERSE_COST, flags)
                    # the goal: the cell nearest (24, 24) that some heading of this footprint fits
                    pose.solve(t_base.data_ptr(), params, fp, np.zeros((0, 3), np.int32), device=True)
                    fits = np.argwhere(pose.layers().any(axis=0))
                    gy, gx = fits[np.argmin(np.abs(fits - (24, 24)).sum(axis=1))]
                    goal = np.array([(gx, gy, -1)], np.int32)
                    places = {"far_corner": (width - WINDOW - 16, height - WINDOW - 16),
                              "half_way": (width // 2 - WINDOW // 2, height // 2 - WINDOW // 2),
                              "next_to_goal": (int(gx) + 8, min(int(gy) + 8, height - WINDOW))}
                    for place, (wx, wy) in places.items():
                        if args.trace and place != "far_corner":
                            continue
                        window = (wx, wy, WINDOW, WINDOW)
                        walled = cost.copy()
                        walled[wy:wy + WINDOW, wx + WINDOW // 2] = 100
                        t_wall = torch.from_numpy(walled).to("cuda:0")
                        torch.cuda.synchronize()
                        seen = {}

                        def start(form):
                            """the handle holds the solve of the base plane, under `form`"""
                            pose.setOption(capi.POSE_OPT_TEST_RESOLVE_FORM, form)
                            seen["base"] = pose.solve(t_base.data_ptr(), params, fp, goal, device=True)

                        def wall(form, into):
                            seen["summary", form, into] = pose.resolve((t_wall if into else t_base).data_ptr(), window, device=True)
                            seen["stats", form, into] = pose.resolveStats()

                        def solve_second():
                            seen["solve"] = second.solve(t_wall.data_ptr(), params, fp, goal, device=True)

                        if args.trace:
                            start(0)
                            wall(0, True), wall(0, False)
                            print(json.dumps({"trace_case": [width, height, share, fp_name, flag_name, place],
                                              "in": seen["stats", 0, True], "out": seen["stats", 0, False]}))
                            return
                        # the two forms leave the same bytes, wall in and wall out
                        same = True
                        kept = {}
                        for form in (1, 0):
                            start(form)
                            for into in (True, False):
                                wall(form, into)
                                got = (pose.potential().tobytes(), pose.floor()[0].tobytes())
                                same = same and kept.setdefault(into, got) == got
                        same = same and all(seen["summary", 0, i] == seen["summary", 1, i] for i in (True, False))
                        del kept
                        per_block = {k: [] for k in ("form0_in_ms", "form0_out_ms", "form1_in_ms", "form1_out_ms", "solve_ms")}

                        def run(form):
                            pose.setOption(capi.POSE_OPT_TEST_RESOLVE_FORM, form)  # (wall in, wall out: the base plane's field again)
                            per_block[f"form{form}_in_ms"].append(timed(pose_stream, lambda: wall(form, True)))
                            per_block[f"form{form}_out_ms"].append(timed(pose_stream, lambda: wall(form, False)))

                        start(0)
                        kinds = [lambda: run(0), lambda: run(1), lambda: per_block["solve_ms"].append(timed(second_stream, solve_second))]
                        for b in range(args.blocks):
                            for k in (kinds if b % 2 == 0 else kinds[::-1]):
                                k()
                        pose.setOption(capi.POSE_OPT_TEST_RESOLVE_FORM, 0)
                        sm = seen["base"]
                        rec = {"width": width, "height": height, "obstacle_share": share, "obstacles": obstacles, "footprint": fp_name,
                               "samples": len(fp), "flags": flag_name, "goal": goal[0].tolist(), "place": place, "window": list(window),
                               "same_bytes_and_summaries": bool(same), "states_reached": sm["states_reached"],
                               "form0_in_stats": seen["stats", 0, True], "form0_out_stats": seen["stats", 0, False],
                               "form1_in_stats": seen["stats", 1, True], "form1_out_stats": seen["stats", 1, False]}
                        rec.update({k: _spread(v) for k, v in per_block.items()})
                        for d in ("in", "out"):
                            rec[f"form1_over_form0_{d}"] = round(statistics.median(per_block[f"form1_{d}_ms"]) /
                                                                 statistics.median(per_block[f"form0_{d}_ms"]), 4)
                        out["runs"].append(rec)
                        save()
                        del t_wall
        del pose, second, clear
    save()
    print(json.dumps({"written": args.out, "runs": len(out["runs"])}))


if __name__ == "__main__":
    main()
