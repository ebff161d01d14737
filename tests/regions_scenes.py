"""Planes for the region grid's tests that tests/navfield_scenes.py does not have (int8, shape (h, w)).  Under the byte
range 100 .. 100 the members of the first four are the cells set to 100."""
import numpy as np


def full(w, h):
    """every cell a member: one region, the hottest record"""
    return np.full((h, w), 100, np.int8)


def empty(w, h):
    return np.zeros((h, w), np.int8)


def dots(w, h):
    """members at even ix and even iy: ceil(w / 2) * ceil(h / 2) regions of one cell under either connectivity"""
    plane = np.zeros((h, w), np.int8)
    plane[0::2, 0::2] = 100
    return plane


def staircase(w, h):
    """the cells (i, i): one region under 8-connectivity, a region per cell under 4-connectivity; every link crosses a
    tile corner where the diagonal does"""
    plane = np.zeros((h, w), np.int8)
    for i in range(min(w, h)):
        plane[i, i] = 100
    return plane


def frontier_plane(w, h, seed=None):
    """a seeded 3-valued occupancy plane: -1 / 0 / 100 at probabilities 0.3 / 0.55 / 0.15"""
    rng = np.random.default_rng(1000 * w + h if seed is None else seed)
    u = rng.random((h, w))
    return np.where(u < 0.3, -1, np.where(u < 0.85, 0, 100)).astype(np.int8)


def room(w=40, h=30):
    """A room of FREE cells inside a grid of UNKNOWN, walled by OCCUPIED cells, with two door gaps that open on UNKNOWN: one
    of 5 cells in the west wall, one of 2 cells in the east wall.  Returns (plane, west gap cells, east gap cells) with the
    cells as sets of (ix, iy)."""
    plane = np.full((h, w), -1, np.int8)
    x0, y0, x1, y1 = 5, 5, w - 6, h - 6
    plane[y0:y1 + 1, x0:x1 + 1] = 100
    plane[y0 + 1:y1, x0 + 1:x1] = 0
    west = {(x0, y) for y in range(10, 15)}
    east = {(x1, y) for y in range(18, 20)}
    for x, y in west | east:
        plane[y, x] = 0
    return plane, west, east
