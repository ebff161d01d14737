#!/usr/bin/env python3
"""What a trajectory rollout costs: one JSON line.
lom_rollout_evaluate_from_grids with the cost plane in HBM -- a ClearanceGrid's, over 2 % seeded obstacles inflated by 0.5 m
-- on two grids of 0.1 m cells, 1174 x 160 and 4096 x 4096, without a potential.  Cases: M = 1 state and K = 8192
candidates (a 64 x 128 lattice of (v, w)) over S = 256 poses as L = 2 x 128 and L = 4 x 64 steps (one segment holds at
most 128 steps, so S = 256 needs two), and over S = 128 as L = 1; M = 64 states and K = 1024; and M = 1, K = 8192 over S
= 64, the one case here whose window of the plane fits the LDS budget.  Each with the perimeter (32 samples) and the
filled (77 samples) footprint of a 1.0 x 0.6 m robot.  Every start state is drawn among those whose filled footprint is
free at pose 0 (step 2 of the definition, restated here in numpy), so every candidate is rolled out at least one step; how
far is recorded per case as the distribution of free_poses over its records, read back from one untimed call under
LOM_ROLLOUT_KEEP_RECORDS.  Two floors are recorded beside them and kept out of the verdict: K = 0, where no evaluation is
launched (upload, fill, summary, read-back), and a start on a lethal cell, where every candidate ends at pose 0 (what the
workgroups' staging of the table and one chunk per candidate cost).  For each, in the same process: the default (a lane per pose, four
waves, the plane read in HBM) against LOM_ROLLOUT_OPT_TEST_SERIAL, the window staged in LDS where it fits
(LOM_ROLLOUT_OPT_TEST_NO_LDS_PLANE = 0) and one wave per workgroup.  HIP events on the handle's stream around the call --
from its enqueue to the end of its read-back -- in --blocks alternating blocks, medians and ranges of the block values;
launches and waits from lom_rollout_stats.  What bounds k_rollout_eval is not stated: that needs counters, collected in a
run of their own.
    python tools/rollout_cost.py [--blocks 5] > profiles/rollout_cost.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(1174, 160), (4096, 4096)]  # width, height
RES = 0.1
LETHAL_MIN = 99
# csrc/rollout_host.hpp: kWindowBudgetBytes, the bytes of the plane a workgroup may stage; a window of side 2 (S + reach) + 1
# cells of a byte fits when its square does, and reach is max ceil((|fx| + |fy|) / 256) + 1 over the footprint's samples
WINDOW_BUDGET_BYTES = 23 << 10
# name, M, K as (speeds, turns), L, Tn, start: "free" -- the footprint is free at pose 0 --, or "blocked" -- the state's own
# cell is lethal, so every candidate ends at t* = 0 and nothing is rolled out: with K = 0 (no evaluation is launched) the
# two floors of a call
CASES = [("m1_k8192_s256_l2", 1, (64, 128), 2, 128, "free"), ("m1_k8192_s256_l4", 1, (64, 128), 4, 64, "free"),
         ("m1_k8192_s128_l1", 1, (64, 128), 1, 128, "free"), ("m64_k1024_s256_l4", 64, (32, 32), 4, 64, "free"),
         ("m1_k8192_s64_l1", 1, (64, 128), 1, 64, "free"), ("floor_m1_k0", 1, (0, 0), 4, 64, "free"),
         ("floor_m1_k8192_blocked_at_pose_0", 1, (64, 128), 4, 64, "blocked")]
VARIANTS = {"default_ms": (-1, -1, 0), "serial_ms": (1, -1, 0), "lds_plane_ms": (-1, 0, 0), "one_wave_ms": (-1, -1, 1)}  # serial, no LDS plane, one wave


def pose0_free(cost, table, footprint, x, y, a):
    """step 2 of the definition at the states themselves, in numpy int64: True where every sample of the footprint lies in
    the grid on a known cell below LETHAL_MIN"""
    import numpy as np
    c, s = table[a >> 4, 0].astype(np.int64)[:, None], table[a >> 4, 1].astype(np.int64)[:, None]
    fx, fy = footprint[:, 0].astype(np.int64)[None, :], footprint[:, 1].astype(np.int64)[None, :]
    cx, cy = (x[:, None] + ((fx * c - fy * s + 128) >> 8)) >> 15, (y[:, None] + ((fx * s + fy * c + 128) >> 8)) >> 15
    inside = (cx >= 0) & (cx < cost.shape[1]) & (cy >= 0) & (cy < cost.shape[0])
    v = cost[np.clip(cy, 0, cost.shape[0] - 1), np.clip(cx, 0, cost.shape[1] - 1)]
    return np.all(inside & (v >= 0) & (v < LETHAL_MIN), axis=1)


def window_fits(steps, footprint):
    reach = max(-(-(abs(int(fx)) + abs(int(fy))) // 256) + 1 for fx, fy in footprint)
    return (2 * (steps + reach) + 1) ** 2 <= WINDOW_BUDGET_BYTES


def _spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


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
           "note": "ms per call, HIP events on the handle's stream, the upload of states, commands and footprint and the read-back "
                   "of picks and summary included; the cost plane in HBM, no potential, no records kept",
           "bound_of_k_rollout_eval": "NOT MEASURED (no counter run): the plane's loads, LDS reads of the footprint, or issue",
           "start_states": [], "runs": []}

    def timed(stream, fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    table = lom.visibilityTable(capi.ROLLOUT_TABLE)
    footprints = {"perimeter": lom.rolloutFootprintRectangle(1280, 1280, 768, 256, True), "filled": lom.rolloutFootprintRectangle(1280, 1280, 768, 256)}
    for width, height in GRIDS:
        rng = np.random.default_rng(width)
        occ = np.where(rng.random((height, width)) < 0.02, 100, 0).astype(np.int8)
        clear = lom.ClearanceGrid(RES, (0.0, 0.0), width, height)
        clear.update(occ, None, (0.5, 0.3, 2.0, 0))
        cost = clear.cost()[0]
        lethal = np.argwhere(cost >= LETHAL_MIN)[:, ::-1]
        # start states: cells of no cost at a random heading, kept where the filled footprint (the perimeter's samples are
        # among its) is free at pose 0
        drawn = np.argwhere(cost == 0)[:, ::-1]
        drawn = drawn[rng.integers(0, len(drawn), 1 << 16)].astype(np.int64)
        drawn = np.stack([drawn[:, 0] * 32768 + 16384, drawn[:, 1] * 32768 + 16384, rng.integers(0, 65536, len(drawn))], axis=1)
        ok = pose0_free(cost, table, footprints["filled"], drawn[:, 0], drawn[:, 1], drawn[:, 2])
        startable = drawn[ok]
        out["start_states"].append({"width": width, "height": height, "lethal_cells": round(len(lethal) / cost.size, 4), "drawn": len(drawn),
                                    "free_at_pose_0": int(ok.sum())})
        dev = lom.RolloutGrid(RES, (0.0, 0.0), width, height)
        stream = torch.cuda.ExternalStream(L.lom_rollout_stream(dev.handle))
        for name, m, (nv, nw), segments, tn, start in CASES:
            if start == "free":
                states, startable = startable[:m], startable[m:]
                assert len(states) == m, "too few start states with a free footprint"
            else:
                cells = lethal[rng.integers(0, len(lethal), m)].astype(np.int64)
                states = np.stack([cells[:, 0] * 32768 + 16384, cells[:, 1] * 32768 + 16384, rng.integers(0, 65536, m)], axis=1)
            v, w = np.meshgrid(np.linspace(-8192, 32767, nv).astype(np.int64), np.linspace(-256, 256, nw).astype(np.int64), indexing="ij")
            cmd = np.stack([np.stack([v.reshape(-1), w.reshape(-1) // (seg + 1)], axis=1) for seg in range(segments)], axis=1).astype(np.int16)
            params = (segments, tn, LETHAL_MIN, -1, 0, 1, 1, 64, 0)
            steps = segments * tn
            for fp_name, fp in footprints.items():
                seen = {}

                def run(kind):
                    serial, no_lds, one_wave = VARIANTS[kind]
                    dev.setOption(capi.ROLLOUT_OPT_TEST_SERIAL, serial)
                    dev.setOption(capi.ROLLOUT_OPT_TEST_NO_LDS_PLANE, no_lds)
                    dev.setOption(capi.ROLLOUT_OPT_TEST_WAVES, 1 if one_wave else 0)
                    ms = timed(stream, lambda: seen.__setitem__(kind, dev.evaluateFromGrids(clear, None, states, cmd, fp, params)))
                    seen[kind + "_stats"] = dev.stats()
                    return ms

                for kind in VARIANTS:
                    run(kind)  # warm-up: code objects, buffers
                first = seen["default_ms"]
                same = all(seen[kind][0].tobytes() == first[0].tobytes() and seen[kind][1] == first[1] for kind in VARIANTS)
                # how far the candidates get: free_poses over the records of one untimed call
                dev.evaluateFromGrids(clear, None, states, cmd, fp, params[:8] + (capi.ROLLOUT_KEEP_RECORDS,))
                t_star = dev.records()["free_poses"].astype(np.int64)
                tested = np.minimum(t_star + 1, steps + 1)  # a serial walk tests poses 0..t*
                reached = {"min": 0, "p25": 0, "median": 0, "p75": 0, "max": 0, "mean": 0.0, "at_pose_0": 0, "never_blocked": 0} if not len(t_star) else {
                    "min": int(t_star.min()), "p25": int(np.percentile(t_star, 25)), "median": int(np.median(t_star)),
                    "p75": int(np.percentile(t_star, 75)), "max": int(t_star.max()), "mean": round(float(t_star.mean()), 2),
                    "at_pose_0": int((t_star == 0).sum()), "never_blocked": int((t_star == steps + 1).sum())}
                names = list(VARIANTS)
                per_block = {kind: [] for kind in names}
                for b in range(args.blocks):
                    for kind in (names if b % 2 == 0 else names[::-1]):
                        per_block[kind].append(run(kind))
                med = {kind: statistics.median(per_block[kind]) for kind in names}
                rec = {"width": width, "height": height, "case": name, "start": start, "states": m, "candidates": len(cmd),
                       "segments": segments, "steps": steps, "footprint": fp_name, "samples": len(fp),
                       "window_fits": bool(window_fits(steps, fp)), "summary": first[1], "stats": seen["default_ms_stats"],
                       "same_bytes": bool(same), "free_poses": reached, "poses_tested_by_a_serial_walk": int(tested.sum()),
                       "plane_reads_upper_bound": int(m * len(cmd) * (steps + 1) * len(fp))}
                rec.update({kind: _spread(per_block[kind]) for kind in names})
                for kind in names[1:]:
                    rec["default_over_" + kind[:-3]] = round(med["default_ms"] / med[kind], 4)
                out["runs"].append(rec)
                print("%d x %d %s %s: default %.3f ms, serial %.3f ms, LDS plane %.3f ms, one wave %.3f ms, same bytes %s" %
                      (width, height, name, fp_name, med["default_ms"], med["serial_ms"], med["lds_plane_ms"], med["one_wave_ms"], same),
                      file=sys.stderr, flush=True)
        for option in (capi.ROLLOUT_OPT_TEST_SERIAL, capi.ROLLOUT_OPT_TEST_NO_LDS_PLANE, capi.ROLLOUT_OPT_TEST_WAVES):
            dev.setOption(option, -1)
        del dev, clear
    # by how much and in how many cases each default wins
    out["verdict"] = {}
    for kind in list(VARIANTS)[1:]:
        runs = [r for r in out["runs"] if r["start"] == "free" and r["candidates"] and (kind != "lds_plane_ms" or r["window_fits"])]
        ratios = [r["default_over_" + kind[:-3]] for r in runs]
        out["verdict"][kind[:-3]] = {"cases": len(ratios), "default_faster_in": sum(x < 1.0 for x in ratios),
                                     "default_over_it": _spread(ratios) if ratios else None,
                                     "default_total_ms": round(sum(r["default_ms"]["median"] for r in runs), 4),
                                     "its_total_ms": round(sum(r[kind]["median"] for r in runs), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
