"""The region grid restated in numpy and Python integers (include/lidar_odometry_amd.h, "frontier regions"): membership,
labels by a flood fill of its own, the records straight from the formulas, the list, the goals, the query and the summary.
tests/test_regions_host.py checks the labels against scipy.ndimage.label and against an all-pairs reachability closure.
Everything is an integer, so every comparison with the device is exact."""
import numpy as np

from tests import navfield_ref as N

NONE, UNREACHED = 0xFFFFFFFF, 0xFFFFFFFF
BYTES, FRONTIER = 0, 1
NEIGHBOURS_8, EDGE_UNKNOWN, CONNECT_4 = 1, 2, 4
RANK_LABEL, RANK_CELLS, RANK_POTENTIAL = 0, 1, 2
GOAL_CENTRE, GOAL_ENTRY = 0, 1
SUMMARY_KEYS = ("cells_member", "regions", "regions_recorded", "regions_listed", "largest_cells")
MAX_REGIONS_DEFAULT = 1 << 20
# lom_regions_record
RECORD = np.dtype([("label", "<u4"), ("cells", "<u4"), ("sum_x", "<u8"), ("sum_y", "<u8"), ("min_x", "<u2"), ("min_y", "<u2"),
                   ("max_x", "<u2"), ("max_y", "<u2"), ("centroid_x", "<u2"), ("centroid_y", "<u2"), ("centre_x", "<u2"),
                   ("centre_y", "<u2"), ("entry_x", "<u2"), ("entry_y", "<u2"), ("entry_potential", "<u4")])
EDGE_STEPS = ((1, 0), (0, 1), (-1, 0), (0, -1))
ALL_STEPS = EDGE_STEPS + ((1, 1), (-1, 1), (-1, -1), (1, -1))


def params(kind, lo=0, hi=0, max_cost=99, min_cells=1, rank=RANK_LABEL, flags=0):
    return dict(kind=int(kind), lo=int(lo), hi=int(hi), max_cost=int(max_cost), min_cells=int(min_cells), rank=int(rank),
                flags=int(flags))


def as_tuple(p):
    return (p["kind"], p["lo"], p["hi"], p["max_cost"], p["min_cells"], p["rank"], p["flags"])


def params_ok(p, have_potential):
    if p["kind"] not in (BYTES, FRONTIER) or not -128 <= p["lo"] <= 127 or not -128 <= p["hi"] <= 127:
        return False
    if p["kind"] == BYTES and p["lo"] > p["hi"]:
        return False
    if not 0 <= p["max_cost"] <= 99 or not 1 <= p["min_cells"] < 1 << 32 or p["flags"] & ~(NEIGHBOURS_8 | EDGE_UNKNOWN | CONNECT_4):
        return False
    if p["rank"] not in (RANK_LABEL, RANK_CELLS, RANK_POTENTIAL):
        return False
    return p["rank"] != RANK_POTENTIAL or have_potential


def members(plane, p, cost=None, potential=None):
    """step 1: a bool array of shape (h, w)"""
    plane = np.asarray(plane, np.int8).astype(int)
    h, w = plane.shape
    if p["kind"] == BYTES:
        m = (plane >= p["lo"]) & (plane <= p["hi"])
    else:
        unknown = np.full((h + 2, w + 2), bool(p["flags"] & EDGE_UNKNOWN))
        unknown[1:-1, 1:-1] = plane == -1
        near = np.zeros((h, w), bool)
        for dx, dy in (ALL_STEPS if p["flags"] & NEIGHBOURS_8 else EDGE_STEPS):
            near |= unknown[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        m = (plane == 0) & near
    if cost is not None:
        c = np.asarray(cost, np.int8).astype(int)
        m &= (c >= 0) & (c <= p["max_cost"])
    if potential is not None:
        m &= np.asarray(potential, np.uint32) != UNREACHED
    return m


def label(m, conn4=False):
    """step 2 by a flood fill in ascending index order: uint32 (h, w), the least linear index of a member's component"""
    h, w = m.shape
    out = np.full((h, w), NONE, np.uint32)
    steps = EDGE_STEPS if conn4 else ALL_STEPS
    seen = np.zeros((h, w), bool)
    for y0, x0 in np.argwhere(m):
        if seen[y0, x0]:
            continue
        lab = int(y0) * w + int(x0)                                   # argwhere is row-major: the first cell met is the least
        stack = [(int(x0), int(y0))]
        seen[y0, x0] = True
        while stack:
            x, y = stack.pop()
            out[y, x] = lab
            for dx, dy in steps:
                nx, ny = x + dx, y + dy
                if 0 <= nx < w and 0 <= ny < h and m[ny, nx] and not seen[ny, nx]:
                    seen[ny, nx] = True
                    stack.append((nx, ny))
    return out


def centroid(total, cells):
    return (2 * int(total) + int(cells)) // (2 * int(cells))


def record_of(lab, labels, potential):
    """step 4 for the region `lab`, from the formulas, on Python integers"""
    h, w = labels.shape
    ys, xs = np.nonzero(labels == lab)
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    cells, sx, sy = len(xs), sum(xs), sum(ys)
    cx, cy = centroid(sx, cells), centroid(sy, cells)
    key, centre = min((((x - cx) ** 2 + (y - cy) ** 2) << 26 | (y * w + x), (x, y)) for x, y in zip(xs, ys))
    assert key >> 26 < 1 << 27
    if potential is None:
        entry, ep = centre, UNREACHED
    else:
        key, entry = min((int(potential[y, x]) << 26 | (y * w + x), (x, y)) for x, y in zip(xs, ys))
        ep = key >> 26
    return (lab, cells, sx, sy, min(xs), min(ys), max(xs), max(ys), cx, cy, centre[0], centre[1], entry[0], entry[1], ep)


def sort_list(records, min_cells, rank):
    """step 5: the records with cells >= min_cells in list order"""
    keep = [r for r in records if int(r["cells"]) >= min_cells]
    if rank == RANK_CELLS:
        keep.sort(key=lambda r: (-int(r["cells"]), int(r["label"])))
    elif rank == RANK_POTENTIAL:
        keep.sort(key=lambda r: (int(r["entry_potential"]), int(r["label"])))
    else:
        keep.sort(key=lambda r: int(r["label"]))
    return np.array(keep, RECORD) if keep else np.zeros(0, RECORD)


def extract(plane, p, cost=None, potential=None, max_regions=MAX_REGIONS_DEFAULT):
    """dict(labels, records, list, summary, error).  A refused extract has error=True and a summary of zeros."""
    zero = dict.fromkeys(SUMMARY_KEYS, 0)
    if not params_ok(p, potential is not None):
        return dict(labels=None, records=None, list=None, summary=zero, error=True)
    pot = None if potential is None else np.asarray(potential, np.uint32)
    m = members(plane, p, cost, pot)
    labels = label(m, bool(p["flags"] & CONNECT_4))
    labs = sorted(int(v) for v in np.unique(labels[m]))
    records = np.zeros(min(len(labs), max_regions), RECORD)
    for k, lab in enumerate(labs[:max_regions]):
        records[k] = record_of(lab, labels, pot)
    lst = sort_list(records, p["min_cells"], p["rank"])
    summary = dict(cells_member=int(m.sum()), regions=len(labs), regions_recorded=len(records), regions_listed=len(lst),
                   largest_cells=int(records["cells"].max()) if len(records) else 0)
    return dict(labels=labels, records=records, list=lst, summary=summary, error=False)


def goals(lst, which):
    """step 6: int32 (n, 2)"""
    a, b = ("centre_x", "centre_y") if which == GOAL_CENTRE else ("entry_x", "entry_y")
    return np.stack([lst[a].astype(np.int32), lst[b].astype(np.int32)], axis=1) if len(lst) else np.zeros((0, 2), np.int32)


def query(geo, labels, xy):
    """step 7: uint32 per point, NONE outside the grid"""
    out = np.full(len(np.asarray(xy).reshape(-1, 2)), NONE, np.uint32)
    for i, cell in enumerate(N.cells_of(geo, xy, True)):
        if cell is not None:
            out[i] = labels[cell[1], cell[0]]
    return out
