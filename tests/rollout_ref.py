"""The trajectory rollouts' definition (include/lidar_odometry_amd.h, "trajectory rollouts") restated: poses(), pose_test()
and evaluate() follow the header step by step on Python integers, one candidate, one pose and one footprint sample at a
time; evaluate_fast() is the same definition over all candidates and poses of a state at once on numpy int64 arrays (every
value stays below 2^42, so it is as exact), for the device tests, whose cases would take minutes pose by pose --
tests/test_rollout_host.py holds the two equal.  The direction table is an argument: the tests pass the library's."""
import numpy as np

KEEP_RECORDS = 1
OK, UNKNOWN, COLLISION, EDGE, INVALID = 0, 1, 2, 3, 4
UNREACHED = 0xFFFFFFFF
NONE = 0xFFFFFFFF
TABLE = 4096
STATE = np.dtype([("x", "<i4"), ("y", "<i4"), ("a", "<u4")])
RECORD = np.dtype([("free_poses", "<u4"), ("reason", "<u4"), ("cost_sum", "<u4"), ("cost_max", "<u4"), ("end_x", "<i4"),
                   ("end_y", "<i4"), ("end_angle", "<u4"), ("end_potential", "<u4")])
PICK = np.dtype([("k", "<u4"), ("admissible", "<u4"), ("score", "<i8")])
SUMMARY_KEYS = ("states", "valid_states", "candidates", "admissible", "states_without_pick")
FIELDS = ("segments", "steps_per_segment", "lethal_min", "unknown_cost", "min_steps", "progress_weight", "cost_weight",
          "truncation_weight", "flags")


def params(segments, steps_per_segment, lethal_min=100, unknown_cost=-1, min_steps=0, progress_weight=1, cost_weight=1,
           truncation_weight=0, flags=KEEP_RECORDS):
    return dict(segments=segments, steps_per_segment=steps_per_segment, lethal_min=lethal_min, unknown_cost=unknown_cost,
                min_steps=min_steps, progress_weight=progress_weight, cost_weight=cost_weight,
                truncation_weight=truncation_weight, flags=flags)


def as_tuple(p):
    return tuple(p[k] for k in FIELDS)


def params_ok(p):
    if not (1 <= p["segments"] <= 8 and 1 <= p["steps_per_segment"] <= 128):
        return False
    S = p["segments"] * p["steps_per_segment"]
    return (S <= 1024 and 1 <= p["lethal_min"] <= 100 and -1 <= p["unknown_cost"] <= 98 and 0 <= p["min_steps"] <= S
            and 0 <= p["progress_weight"] <= 256 and 0 <= p["cost_weight"] <= 4096 and 0 <= p["truncation_weight"] <= 1 << 20
            and p["flags"] & ~KEEP_RECORDS == 0)


def inputs_ok(states, commands, footprint, p):
    """the ranges of the states (M, 3), the commands (K, L, 2) and the footprint (F, 2)"""
    m, k, f = len(states), len(commands), len(footprint)
    if not (m <= 4096 and k <= 1 << 20 and m * k <= 1 << 22 and 1 <= f <= 1024):
        return False
    if any(not (-(1 << 29) <= x < 1 << 29 and -(1 << 29) <= y < 1 << 29 and 0 <= a < 65536) for x, y, a in states):
        return False
    return all(abs(int(fx)) <= 16384 and abs(int(fy)) <= 16384 for fx, fy in footprint)


def numpy_table():
    """the table with numpy's cos and sin (the library's entries lie within 1 of these)"""
    a = 2.0 * np.pi * np.arange(TABLE) / TABLE
    return np.stack([np.rint(np.cos(a) * 32768.0), np.rint(np.sin(a) * 32768.0)], axis=1).astype(np.int32)


# ---- pose by pose, on Python integers ---------------------------------------------------------------------------------------
def poses(p, state, commands, table):
    """step 1: the S + 1 poses (x, y, a) of one candidate; commands: L pairs (v, w)"""
    x, y, a = (int(v) for v in state)
    out = [(x, y, a)]
    for t in range(p["segments"] * p["steps_per_segment"]):
        v, w = (int(c) for c in commands[t // p["steps_per_segment"]])
        b = a >> 4
        x += (v * int(table[b][0]) + 16384) >> 15
        y += (v * int(table[b][1]) + 16384) >> 15
        a = (a + w) & 65535
        out.append((x, y, a))
    return out


def pose_test(plane, pose, footprint, table, p):
    """step 2: (the pose's code, its cost)"""
    h, w = plane.shape
    x, y, a = pose
    c, s = int(table[a >> 4][0]), int(table[a >> 4][1])
    code, cost = OK, 0
    for fx, fy in footprint:
        fx, fy = int(fx), int(fy)
        cx = (x + ((fx * c - fy * s + 128) >> 8)) >> 15
        cy = (y + ((fx * s + fy * c + 128) >> 8)) >> 15
        if not (0 <= cx < w and 0 <= cy < h):
            sample, sample_cost = EDGE, 0
        else:
            v = int(plane[cy, cx])
            if v >= p["lethal_min"]:
                sample, sample_cost = COLLISION, 0
            elif v < 0 and p["unknown_cost"] < 0:
                sample, sample_cost = UNKNOWN, 0
            else:
                sample, sample_cost = OK, p["unknown_cost"] if v < 0 else v
        code, cost = max(code, sample), max(cost, sample_cost)
    return code, cost


def _potential_at(potential, x, y):
    if potential is None:
        return UNREACHED
    h, w = potential.shape
    cx, cy = x >> 15, y >> 15
    return int(potential[cy, cx]) if 0 <= cx < w and 0 <= cy < h else UNREACHED


def record_of(plane, potential, state, commands, footprint, table, p):
    """step 3 for one state and candidate, as a tuple in RECORD's order"""
    h, w = plane.shape
    x0, y0, a0 = (int(v) for v in state)
    if not (0 <= x0 >> 15 < w and 0 <= y0 >> 15 < h):
        return (0, INVALID, 0, 0, x0, y0, a0, UNREACHED)
    S = p["segments"] * p["steps_per_segment"]
    free, reason, cost_sum, cost_max, end = S + 1, OK, 0, 0, (x0, y0, a0)
    for t, pose in enumerate(poses(p, state, commands, table)):
        code, cost = pose_test(plane, pose, footprint, table, p)
        if code != OK:
            free, reason = t, code
            break
        cost_sum, cost_max, end = cost_sum + cost, max(cost_max, cost), pose
    return (free, reason, cost_sum, cost_max, end[0], end[1], end[2], _potential_at(potential, end[0], end[1]))


def _score(p, potential, p0, rec):
    """step 4: the score, or None where the candidate is not admissible"""
    free, _, cost_sum, _, _, _, _, end_potential = (int(v) for v in rec)
    if free <= p["min_steps"] or (potential is not None and (p0 == UNREACHED or end_potential == UNREACHED)):
        return None
    S = p["segments"] * p["steps_per_segment"]
    progress = p["progress_weight"] * (p0 - end_potential) if potential is not None else 0
    return progress - p["cost_weight"] * cost_sum - p["truncation_weight"] * (S + 1 - free)


def _finish(plane, potential, states, records, p, k):
    """steps 4 and 5 from the records (M, K)"""
    h, w = plane.shape
    m = len(states)
    picks = np.zeros(m, PICK)
    valid = admissible = none = 0
    for i, (x, y, _) in enumerate(states):
        x, y = int(x), int(y)
        valid += 0 <= x >> 15 < w and 0 <= y >> 15 < h
        p0 = _potential_at(potential, x, y)
        best, count = None, 0
        for j in range(k):
            s = _score(p, potential, p0, records[i * k + j])
            if s is not None:
                assert abs(s) < 1 << 41
                count += 1
                if best is None or s > best[1]:                    # ties: the least k stays
                    best = (j, s)
        picks[i] = (NONE, 0, 0) if best is None else (best[0], count, best[1])
        admissible += count
        none += best is None
    summary = dict(states=m, valid_states=int(valid), candidates=m * k, admissible=admissible, states_without_pick=int(none))
    return dict(records=records, picks=picks, summary=summary, error=False)


def _refused(m):
    return dict(records=np.zeros(0, RECORD), picks=np.zeros(min(m, 4096), PICK), summary=dict.fromkeys(SUMMARY_KEYS, 0), error=True)


def _inputs(plane, potential, states, commands, footprint, p):
    plane = np.asarray(plane, np.int8)
    potential = None if potential is None else np.asarray(potential, np.uint32)
    states = np.asarray(states, np.int64).reshape(-1, 3)
    commands = np.asarray(commands, np.int64)
    commands = commands.reshape(len(commands), -1, 2) if len(commands) else np.zeros((0, max(p["segments"], 1), 2), np.int64)
    footprint = np.asarray(footprint, np.int64).reshape(-1, 2)
    ok = params_ok(p) and inputs_ok(states.tolist(), commands, footprint.tolist(), p)
    assert not ok or not len(commands) or commands.shape[1] == p["segments"]
    return plane, potential, states, commands, footprint, ok


def evaluate(plane, potential, states, commands, footprint, table, p):
    """dict(records RECORD (M * K), picks PICK (M), summary, error).  A refused call has error=True, zeroed picks and summary."""
    plane, potential, states, commands, footprint, ok = _inputs(plane, potential, states, commands, footprint, p)
    if not ok:
        return _refused(len(states))
    k = len(commands)
    records = np.zeros(len(states) * k, RECORD)
    for i, st in enumerate(states):
        for j in range(k):
            records[i * k + j] = record_of(plane, potential, st, commands[j], footprint, table, p)
    return _finish(plane, potential, states, records, p, k)


# ---- all candidates and poses of a state at once, on numpy int64 -------------------------------------------------------------
def evaluate_fast(plane, potential, states, commands, footprint, table, p):
    """evaluate(), vectorised"""
    plane, potential, states, commands, footprint, ok = _inputs(plane, potential, states, commands, footprint, p)
    if not ok:
        return _refused(len(states))
    h, w = plane.shape
    k, tn = len(commands), p["steps_per_segment"]
    S = p["segments"] * tn
    tab = np.asarray(table, np.int64)
    pv = plane.astype(np.int64)
    records = np.zeros(len(states) * k, RECORD)
    ar = np.arange(k)
    for i, (x0, y0, a0) in enumerate(states.tolist()):
        rec = records[i * k:(i + 1) * k]
        if not (0 <= x0 >> 15 < w and 0 <= y0 >> 15 < h):
            rec["reason"], rec["end_x"], rec["end_y"], rec["end_angle"], rec["end_potential"] = INVALID, x0, y0, a0, UNREACHED
            continue
        if not k:
            continue
        v, wt = np.repeat(commands[:, :, 0], tn, axis=1), np.repeat(commands[:, :, 1], tn, axis=1)             # (K, S)
        a = np.concatenate([np.full((k, 1), a0, np.int64), a0 + np.cumsum(wt, axis=1)], axis=1) & 65535       # (K, S + 1)
        c, s = tab[a >> 4, 0], tab[a >> 4, 1]
        zero = np.zeros((k, 1), np.int64)
        x = x0 + np.concatenate([zero, np.cumsum((v * c[:, :S] + 16384) >> 15, axis=1)], axis=1)
        y = y0 + np.concatenate([zero, np.cumsum((v * s[:, :S] + 16384) >> 15, axis=1)], axis=1)
        code, cost = np.zeros((k, S + 1), np.int64), np.zeros((k, S + 1), np.int64)
        for fx, fy in footprint.tolist():
            cx = (x + ((fx * c - fy * s + 128) >> 8)) >> 15
            cy = (y + ((fx * s + fy * c + 128) >> 8)) >> 15
            inside = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
            val = pv[np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)]
            lethal, unknown = val >= p["lethal_min"], val < 0
            sample = np.where(~inside, EDGE, np.where(lethal, COLLISION, np.where(unknown & (p["unknown_cost"] < 0), UNKNOWN, OK)))
            code = np.maximum(code, sample)
            cost = np.maximum(cost, np.where(sample == OK, np.where(unknown, p["unknown_cost"], val), 0))
        blocked = code != OK
        any_blocked = blocked.any(axis=1)
        free = np.where(any_blocked, blocked.argmax(axis=1), S + 1)
        below = np.arange(S + 1)[None, :] < free[:, None]
        end = np.maximum(free - 1, 0)
        ex, ey = x[ar, end], y[ar, end]
        rec["free_poses"], rec["reason"] = free, np.where(any_blocked, code[ar, np.minimum(free, S)], OK)
        rec["cost_sum"], rec["cost_max"] = (cost * below).sum(axis=1), (cost * below).max(axis=1)
        rec["end_x"], rec["end_y"], rec["end_angle"] = ex, ey, a[ar, end]
        if potential is None:
            rec["end_potential"] = UNREACHED
        else:
            ecx, ecy = ex >> 15, ey >> 15
            inside = (ecx >= 0) & (ecx < w) & (ecy >= 0) & (ecy < h)
            rec["end_potential"] = np.where(inside, potential[np.clip(ecy, 0, h - 1), np.clip(ecx, 0, w - 1)], UNREACHED)
    return _finish(plane, potential, states, records, p, k)


# ---- the host-only helpers --------------------------------------------------------------------------------------------------
def footprint_rectangle(front, back, half_width, spacing, perimeter_only=False):
    """(F, 2) int32, all in 1/256 cell: the lattice xs x ys, x-major, or its border rows and columns"""
    def axis(lo, hi):
        out, a = [], -lo
        while a < hi:
            out.append(a)
            a += spacing
        return out + [hi]

    xs, ys = axis(back, front), axis(half_width, half_width)
    pts = [(x, y) for i, x in enumerate(xs) for j, y in enumerate(ys)
           if not perimeter_only or i in (0, len(xs) - 1) or j in (0, len(ys) - 1)]
    return np.array(pts, np.int32).reshape(-1, 2)


def state_from_pose(geo, x_m, y_m, yaw):
    """(x, y, a) with numpy f64, or None where the library refuses"""
    vals = np.array([x_m, y_m, yaw], np.float32).astype(np.float64)
    if not np.isfinite(vals).all():
        return None
    r, ox, oy = (np.float64(np.float32(geo[k])) for k in ("resolution", "origin_x", "origin_y"))
    x, y = np.floor((vals[0] - ox) / r * 32768.0), np.floor((vals[1] - oy) / r * 32768.0)
    if not (-(1 << 29) <= x < 1 << 29 and -(1 << 29) <= y < 1 << 29):
        return None
    turns = vals[2] / (2.0 * np.pi) * 65536.0
    if not abs(turns) < 9.0e18:                                                  # beyond llround's range
        return None
    rounded = int(np.sign(turns) * np.floor(np.abs(turns) + 0.5))                # llround: halves away from zero
    return int(x), int(y), rounded & 65535
