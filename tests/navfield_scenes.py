"""Cost planes for the navigation field's tests (int8, shape (h, w), the value range of lom_clearance_cost): 0 is free
ground, 100 an obstacle, -1 unknown."""
import numpy as np


def empty(w, h):
    return np.zeros((h, w), np.int8)


def random_plane(rng, w, h, obstacles=0.3, unknown=0.1):
    """`obstacles` of the cells lethal, `unknown` of them -1, the rest random costs 0 .. 98 (and a few 99)"""
    plane = rng.integers(0, 99, (h, w)).astype(np.int8)
    u = rng.random((h, w))
    plane[u < obstacles] = 100
    plane[(u >= obstacles) & (u < obstacles + unknown)] = -1
    plane[rng.random((h, w)) < 0.01] = 99
    return plane


def serpentine(w, h):
    """one-cell corridors along x on the even rows, joined at alternating ends: one route through every tile, many times"""
    plane = np.full((h, w), 100, np.int8)
    plane[0::2, :] = 0
    for k, y in enumerate(range(1, h, 2)):
        plane[y, w - 1 if k % 2 == 0 else 0] = 0
    return plane


def spiral(w, h):
    """a one-cell corridor that winds inwards from (0, 0), walls one cell thick"""
    plane = np.full((h, w), 100, np.int8)
    x0, y0, x1, y1 = 0, 0, w - 1, h - 1
    x, y = 0, 0
    plane[y, x] = 0
    while x0 <= x1 and y0 <= y1:
        for tx, ty in ((x1, y0), (x1, y1), (x0, y1), (x0, y0 + 2)):
            # walk the straight leg to (tx, ty)
            while (x, y) != (tx, ty):
                if x != tx and y != ty:
                    return plane          # the spiral has closed in on itself
                x += (tx > x) - (tx < x)
                y += (ty > y) - (ty < y)
                if not (0 <= x < w and 0 <= y < h):
                    return plane
                plane[y, x] = 0
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
        if x0 > x1 or y0 > y1:
            break
    return plane


def diagonal_gaps(w, h):
    """free ground with pairs of obstacles that touch at a corner only -- the diagonal between them must not be taken -- in
    the middle of a tile, across the tile corner at (31, 31) / (32, 32), and at the grid's edges"""
    plane = np.zeros((h, w), np.int8)

    def pair(x, y, flip=False):
        for px, py in (((x, y + 1), (x + 1, y)) if flip else ((x, y), (x + 1, y + 1))):
            if 0 <= px < w and 0 <= py < h:
                plane[py, px] = 100

    for x, y, flip in ((5, 5, False), (9, 3, True), (31, 31, False), (31, 31 - 4, True), (63, 31, True), (0, 0, True),
                       (w - 2, h - 2, False), (w - 2, 0, False), (0, h - 2, True)):
        pair(x, y, flip)
    # a wall whose only opening is such a corner: two long bars that meet diagonally
    if w >= 8 and h >= 8:
        plane[h // 2, : w // 2] = 100
        plane[h // 2 + 1, w // 2:] = 100
    return plane


def pocket(w, h):
    """free ground with a closed box of obstacles whose inside is free: unreached from outside"""
    plane = np.zeros((h, w), np.int8)
    x0, y0 = w // 3, h // 3
    x1, y1 = min(x0 + max(w // 3, 2), w - 1), min(y0 + max(h // 3, 2), h - 1)
    plane[y0:y1 + 1, x0:x1 + 1] = 100
    plane[y0 + 1:y1, x0 + 1:x1] = 0
    return plane


def two_rooms(w, h, door_y):
    """a wall at x = w // 2 from top to bottom with one door cell"""
    plane = np.zeros((h, w), np.int8)
    plane[:, w // 2] = 100
    plane[door_y, w // 2] = 0
    return plane
