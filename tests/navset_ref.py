"""The navigation field set restated on tests/navfield_ref.py (include/lidar_odometry_amd.h, "navigation field set"): N
solves of the single field, the gather, the nearest-goal partition and the paths on a named field.  Everything is an
integer, so every comparison with the device is exact."""
import numpy as np

from tests import navfield_ref as N

NO_OWNER = 0xFFFF
MAX_FIELDS = 65535
MAX_GOALS = 1 << 24


def offsets_of(goals_per_field):
    """(all goals (n, 2), offsets (n_fields + 1,)) as lom_navset_solve takes them"""
    per = [np.asarray(g).reshape(-1, 2) for g in goals_per_field]
    offsets = np.zeros(len(per) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(g) for g in per])
    return (np.concatenate(per) if per else np.zeros((0, 2), np.int32)), offsets


def offsets_ok(offsets, n_fields, max_fields, have_goals=True):
    """the offsets rule: n_fields <= max_fields; with fields, n_fields + 1 values that start at 0, never fall and end at
    n_goals <= 2^24, with a goal array where n_goals > 0"""
    if n_fields > max_fields:
        return False
    if n_fields == 0:
        return True
    if offsets is None or len(offsets) < n_fields + 1 or int(offsets[0]) != 0:
        return False
    o = [int(v) for v in offsets[:n_fields + 1]]
    if any(b < a for a, b in zip(o, o[1:])) or o[-1] > MAX_GOALS:
        return False
    return have_goals or o[-1] == 0


def solve_set(geo, plane, p, goals_per_field, metres=False):
    """a list of N.solve results, one per field"""
    return [N.solve(geo, plane, p, np.asarray(g).reshape(-1, 2), metres) for g in goals_per_field]


def gather(geo, fields, points, metres=False):
    """uint32 (n_fields, n): P of every field at every point, UNREACHED outside the grid"""
    cells = N.cells_of(geo, points, metres)
    out = np.full((len(fields), len(cells)), N.UNREACHED, np.uint32)
    for i, f in enumerate(fields):
        for j, cell in enumerate(cells):
            if cell is not None:
                out[i, j] = f["P"][cell[1], cell[0]]
    return out


def nearest(geo, fields):
    """(owner uint16 (h, w), potential uint32 (h, w), cells_owned uint64 (n_fields,)): per cell the least P over the
    fields and the least index that attains it; NO_OWNER and UNREACHED where no field reaches the cell"""
    h, w = geo["height"], geo["width"]
    owner, potential = np.full((h, w), NO_OWNER, np.uint16), np.full((h, w), N.UNREACHED, np.uint32)
    owned = np.zeros(len(fields), np.uint64)
    if fields:
        stack = np.stack([f["P"] for f in fields])
        potential = stack.min(axis=0)
        who = stack.argmin(axis=0)                      # (the first of equal values: the least index)
        owner = np.where(potential == N.UNREACHED, NO_OWNER, who).astype(np.uint16)
        owned = np.bincount(owner[owner != NO_OWNER].astype(np.int64), minlength=len(fields)).astype(np.uint64)
    return owner, potential, owned


def paths(geo, fields, field_of_start, starts, cap, metres=False):
    """(cells uint16 (K, cap, 2), lengths uint32 (K,)): N.paths' walk, start k down field field_of_start[k]; None where an
    index is outside the fields (the device refuses the call)"""
    starts = np.asarray(starts).reshape(-1, 2)
    if any(not 0 <= int(i) < len(fields) for i in field_of_start):
        return None
    cells, lengths = np.zeros((len(starts), cap, 2), np.uint16), np.zeros(len(starts), np.uint32)
    for k, i in enumerate(field_of_start):
        c, n = N.paths(geo, fields[int(i)]["costs"], fields[int(i)]["P"], starts[k:k + 1], cap, metres)
        cells[k], lengths[k] = c[0], n[0]
    return cells, lengths
