"""Commands, states and footprints for the trajectory rollouts' tests."""
import numpy as np

CELL = 32768


def commands_of(rng, k, segments):
    """(K, L, 2) int16: random commands, with v = 0 and w != 0, a negative v, +-32767, a w that wraps the angle past 65536
    within a few steps and a standing candidate among them; the last repeats the first (a tie in every score)"""
    cmd = np.stack([rng.integers(-32767, 32768, (k, segments)), rng.integers(-3000, 3001, (k, segments))], axis=2).astype(np.int16)
    special = [(0, 777), (-20000, -100), (32767, 0), (-32767, 5), (12000, 30000), (9000, -32768), (0, 0)]
    for j, (v, w) in enumerate(special[:k]):
        cmd[j, :, 0], cmd[j, :, 1] = v, w
    if k > len(special) + 1:
        cmd[-1] = cmd[len(special)]
        cmd[len(special):, :, 0] //= 8                                           # slow: many keep all their poses
    return cmd


def states_of(plane, rng, m):
    """(m, 3) int64, alternating between random states on cells a run can start from (anywhere, where there is none) and
    special states -- the corner cell at its outer corner, a state one unit outside the grid, one on a lethal cell where
    the plane has one, the far corner, the other sides and corners, one far outside"""
    h, w = plane.shape
    special = [(0, 0, 0), (-1, (h // 2) * CELL, 100), (w * CELL - 1, h * CELL - 1, 32768), ((w // 2) * CELL, -1, 16384),
               (w * CELL, 5, 65535), (3, h * CELL, 49152), (-(1 << 29), (1 << 29) - 1, 7), (w * CELL - 1, 0, 8192), (0, h * CELL - 1, 40000)]
    lethal = np.argwhere(plane >= 100)
    if len(lethal):
        y, x = lethal[len(lethal) // 2]
        special.insert(2, (int(x) * CELL + 100, int(y) * CELL + 200, 3000))
    free = np.argwhere((plane >= 0) & (plane < 50))
    if not len(free):
        free = np.argwhere(plane > -200)
    st = []
    for i in range(m):
        if i % 2 == 1 and i // 2 < len(special):
            st.append(special[i // 2])
        else:
            y, x = free[int(rng.integers(0, len(free)))]
            st.append((int(x) * CELL + int(rng.integers(0, CELL)), int(y) * CELL + int(rng.integers(0, CELL)), int(rng.integers(0, 65536))))
    return np.array(st, np.int64).reshape(-1, 3)


def footprint_of(rng, f, extent=200):
    """(f, 2) int64 in 1/256 cell: the origin first, then random samples within +-extent"""
    fp = rng.integers(-extent, extent + 1, (f, 2))
    fp[0] = (0, 0)
    return fp
