#!/usr/bin/env python3
"""Throughput of place recognition: one JSON line, also written to profiles/place_throughput.json.

Shape (R, S) = (20, 60).  Three databases of 100,000 seeded descriptors, one per value of E (entries a wave of
k_place_query works on per LDS read).  The library ships E = 8 alone; the comparison needs the measuring build
(`make -C lidar_odometry_demo_amd/csrc tune` -> liblidar_odometry_amd_tune.so, the same sources with
-DLOM_PLACE_TUNE, where LOM_PLACE_QUERY_ENTRIES = 8, 4, 1 at create chooses E), which this tool loads when it is
there; without it E = 8 alone is timed.
    query      wall time per lom_place_db_query call (k = 10, ctypes call included) on the id ranges [0, N) for
               N = 1,000, 10,000 and 100,000 at Q = 1 and Q = 16; five blocks per E, the three E alternating
    numpy      the same query for ONE descriptor in vectorised numpy f32 on the CPUs of the box (a baseline for the
               reader, not a bar)
    describe   lom_place_describe_device on a 26,600-point frame in HBM, by HIP events on the database's stream
    bound      what the kernel's own instruction mix gives for a (query, entry) pair at E: R S wave64 FMAs (a lane
               per shift) at 2 cycles each on one of the CU's four SIMDs, and R S / E ds_read_b32 at 2 LDS cycles
               each per CU; at the NOMINAL 2.4 GHz (the clock under load was not measured)
    python tools/place_throughput.py [--blocks 5] [--entries 100000]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

R, S = 20, 60
PARAMS = (R, S, 80.0, -2.0)
CUS, SIMDS, GHZ = 256, 4, 2.4


def _spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2), "n": len(xs)}


def descriptors(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.random((n, R, S), dtype=np.float32) * 3.0
    d[rng.random((n, R, S)) < 0.15] = 0.0
    d[rng.random((n, 1, S)).repeat(R, axis=1) < 0.05] = 0.0
    return d


def numpy_query(q, unit, mask, k):
    """f32, vectorised: cosines of all column pairs by one matrix product per chunk, then the S diagonals"""
    n = len(unit)
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(axis=0))
    qu = np.where(qn > 0, q / np.where(qn > 0, qn, 1), 0).astype(np.float32)  # [R, S]
    qm = qn > 0
    j = np.arange(S)
    idx = np.stack([((j + s) % S) * S + j for s in range(S)])  # [s, j] -> flat (column of the entry, column of the query)
    best = np.empty(n, np.float32)
    for a in range(0, n, 4096):
        cu = unit[a:a + 4096]  # [c, S, R]
        M = (cu.reshape(-1, R) @ qu).reshape(len(cu), S * S)
        both = (mask[a:a + 4096, :, None] & qm[None, None, :]).reshape(len(cu), S * S)
        tot = np.where(both[:, idx], M[:, idx], np.float32(0)).sum(axis=2)
        cnt = both[:, idx].sum(axis=2)
        d = np.where(cnt > 0, np.float32(1) - tot / np.maximum(cnt, 1).astype(np.float32), np.float32(1))
        best[a:a + 4096] = d.min(axis=1)
    return np.argsort(best, kind="stable")[:k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--entries", type=int, default=100000)
    args = ap.parse_args()
    blocks = max(5, args.blocks)
    tune = os.path.join(ROOT, "lidar_odometry_demo_amd", "liblidar_odometry_amd_tune.so")
    have_tune = os.path.exists(tune) and not os.environ.get("LOM_LIB_PATH")
    if have_tune:
        os.environ["LOM_LIB_PATH"] = tune
    import lidar_odometry_demo_amd as lom
    from lidar_odometry_demo_amd import capi

    L = capi.lib()
    if L.lom_device_count() < 1:
        raise SystemExit("place_throughput needs a GPU: no HIP device visible")
    es = (8, 4, 1) if have_tune else (8,)
    sizes = [n for n in (1000, 10000, 100000) if n <= args.entries]
    entries = descriptors(args.entries, 1)
    queries = descriptors(16, 2)
    dbs = {}
    for E in es:
        os.environ["LOM_PLACE_QUERY_ENTRIES"] = str(E)
        db = lom.PlaceDatabase(PARAMS, capacity_hint=args.entries)
        for d in entries:
            db.add(d)
        dbs[E] = db
    os.environ.pop("LOM_PLACE_QUERY_ENTRIES")
    out = {"shape": [R, S], "k": 10, "measuring_build": have_tune, "entries": args.entries, "blocks_each": blocks,
           "commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None,
           "note": "wall us per lom_place_db_query call incl. the ctypes call; medians and ranges over alternating blocks",
           "query": {}, "numpy_f32_one_query": {}}
    match = np.zeros((16, 10), capi.PLACE_MATCH)
    first = {}
    for n in sizes:
        for Q in (1, 16):
            qd = np.ascontiguousarray(queries[:Q])
            us = {E: [] for E in dbs}

            def call(E):
                capi.check(L.lom_place_db_query(dbs[E].handle, qd.ctypes.data, Q, 0, n, 10, match.ctypes.data, None))

            for E in dbs:
                call(E)
                first.setdefault((n, Q), match[:Q].copy())
                assert match[:Q].tobytes() == first[(n, Q)].tobytes(), "the three E give the same bytes"
            reps = max(3, min(200, int(2e5 / n)))
            for b in range(blocks):
                order = list(es) if b % 2 == 0 else list(es)[::-1]
                for E in order:
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        call(E)
                    us[E].append((time.perf_counter() - t0) / reps * 1e6)
            row = {}
            for E in dbs:
                med = statistics.median(us[E])
                fma_us = n * Q * (R * S * 2.0) / (CUS * SIMDS) / (GHZ * 1e3)
                lds_us = n * Q * (R * S / E * 2.0) / CUS / (GHZ * 1e3)
                row["E%d" % E] = {"us_per_call": _spread(us[E]), "ns_per_pair": round(med * 1e3 / (n * Q), 3),
                                  "bound_fma_us": round(fma_us, 2), "bound_lds_us": round(lds_us, 2),
                                  "bound": "LDS issue" if lds_us > fma_us else "FMA issue",
                                  "fraction_of_bound": round(max(fma_us, lds_us) / med, 3), "calls_per_block": reps}
            out["query"]["N%d_Q%d" % (n, Q)] = row
    # the CPU baseline: one query, the entries' unit columns prepared beforehand (as the database keeps them)
    norm = np.sqrt((entries.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
    unit = np.where(norm > 0, entries / np.where(norm > 0, norm, 1), 0).astype(np.float32).transpose(0, 2, 1).copy()
    mask = norm[:, 0, :] > 0
    for n in sizes:
        numpy_query(queries[0], unit[:n], mask[:n], 10)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            top = numpy_query(queries[0], unit[:n], mask[:n], 10)
            ts.append((time.perf_counter() - t0) * 1e3)
        gpu = dbs[8].query(queries[0], k=10, id_end=n)
        out["numpy_f32_one_query"]["N%d" % n] = {"ms": _spread(ts), "cpus": len(os.sched_getaffinity(0)),
                                                 "top10_equal_to_device": bool(np.array_equal(top, gpu["id"][0]))}
    # describe_device on a frame in HBM, by HIP events on the database's stream
    rng = np.random.default_rng(3)
    frame = np.zeros((26600, 8), np.float32)
    frame[:, :2] = rng.uniform(-70, 70, (26600, 2))
    frame[:, 2] = rng.uniform(-2.5, 6, 26600)
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    L.hipEventSynchronize.argtypes = [C.c_void_p]
    L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    L.hipFree.argtypes = [C.c_void_p]
    d_frame, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.hipMalloc(C.byref(d_frame), frame.nbytes) == 0 and L.hipMemcpy(d_frame, frame.ctypes.data, frame.nbytes, 1) == 0
    assert L.hipEventCreate(C.byref(e0)) == 0 and L.hipEventCreate(C.byref(e1)) == 0
    db = dbs[8]
    stream = L.lom_place_db_stream(db.handle)
    desc = np.empty((R, S), np.float32)
    ev_us, wall_us = [], []
    for i in range(60):
        t0 = time.perf_counter()
        L.hipEventRecord(e0, stream)
        capi.check(L.lom_place_describe_device(db.handle, d_frame, len(frame), 32, desc.ctypes.data))
        L.hipEventRecord(e1, stream)
        L.hipEventSynchronize(e1)
        wall_us.append((time.perf_counter() - t0) * 1e6)
        ms = C.c_float()
        L.hipEventElapsedTime(C.byref(ms), e0, e1)
        if i >= 10:
            ev_us.append(ms.value * 1e3)
    out["describe_device_26600_points"] = {"event_us": _spread(ev_us), "wall_us_incl_events": _spread(wall_us[10:]),
                                           "non_zero_cells": int((desc > 0).sum())}
    L.hipFree(d_frame)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "place_throughput.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
