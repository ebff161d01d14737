"""Cost planes and footprints for the pose field's tests.  Planes are int8 of shape (h, w) in the value range of
lom_clearance_cost: 0 is free ground, 100 an obstacle, -1 unknown; the navigation field's scenes are reused.  Footprints
are (F, 2) int32 samples in 1/256 cell in the robot's frame, +x ahead."""
import numpy as np

from tests import navfield_scenes as S

empty, serpentine, spiral, diagonal_gaps, pocket = S.empty, S.serpentine, S.spiral, S.diagonal_gaps, S.pocket


def all_blocked(w, h):
    return np.full((h, w), 100, np.int8)


def sparse(rng, w, h, obstacles):
    """free ground of random costs 0 .. 40 with `obstacles` of the cells lethal"""
    plane = rng.integers(0, 41, (h, w)).astype(np.int8)
    plane[rng.random((h, w)) < obstacles] = 100
    return plane


def with_unknown_and_invalid(rng, w, h):
    """sparse at 2 %, with 3 % of the cells -1 and a few bytes outside -1 .. 100"""
    plane = sparse(rng, w, h, 0.02)
    u = rng.random((h, w))
    plane[u < 0.03] = -1
    plane[(u >= 0.03) & (u < 0.04)] = rng.choice(np.array([-128, -2, 101, 127], np.int8), int(((u >= 0.03) & (u < 0.04)).sum()))
    return plane


def l_corridor(w, h, width):
    """an L-shaped corridor `width` cells wide in solid rock: one arm along x near the bottom, one along y near the right;
    returns (plane, a cell in the middle of the x arm's far end, a cell in the middle of the y arm's far end)"""
    plane = np.full((h, w), 100, np.int8)
    m = 3                                  # rock left around the corridor
    x1 = w - m                             # the corridor's right edge (exclusive)
    plane[m:m + width, m:x1] = 0           # the arm along x
    plane[m:h - m, x1 - width:x1] = 0      # the arm along y
    half = width // 2
    return plane, (m + 6, m + half), (x1 - width + half, h - m - 7)


def doorway(w, h, door=3):
    """free ground cut by a wall one cell thick at x = w // 2 with one opening `door` cells wide around y = h // 2; returns
    (plane, the opening's centre cell)"""
    plane = np.zeros((h, w), np.int8)
    plane[:, w // 2] = 100
    y0 = h // 2 - door // 2
    plane[y0:y0 + door, w // 2] = 0
    return plane, (w // 2, h // 2)


# ---- footprints ------------------------------------------------------------------------------------------------------------
POINT = np.zeros((1, 2), np.int32)


def rectangle(front, back, half_width, spacing):
    """the lattice of lom_rollout_footprint_rectangle: xs = -back, -back + spacing, ... while < front, then front; ys likewise"""
    def axis(lo, hi):
        return list(range(-lo, hi, spacing)) + [hi]
    return np.array([(x, y) for x in axis(back, front) for y in axis(half_width, half_width)], np.int32)


def rect_cells(length, width, spacing=128):
    """a filled rectangle that covers length x width cells (both odd) at heading 0, sampled every `spacing` / 256 cell"""
    return rectangle((length // 2) * 256, (length // 2) * 256, (width // 2) * 256, spacing)


RECT_5x3 = rect_cells(5, 3)
RECT_9x3 = rect_cells(9, 3)
# an asymmetric L: a 5-cell spine ahead of the centre and a 2-cell foot to the left at its rear
L_SHAPE = np.array([(x, 0) for x in range(-256, 1025, 128)] + [(-256, y) for y in range(128, 513, 128)], np.int32)


def big(rng):
    """F = 1024 samples within a 7 x 5-cell box"""
    return np.stack([rng.integers(-768, 769, 1024), rng.integers(-512, 513, 1024)], axis=1).astype(np.int32)
