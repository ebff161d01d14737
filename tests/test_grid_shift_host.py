"""The rule of the grid shift on the host: lom_grid_shift_geometry and lom_grid_follow of the built library against
tests/grid_shift_ref.py -- bits of the shifted origins, every refusal, and lom_grid_follow for every side from 2 to 40, every
admissible margin and quantum and every cell from -200 to 239, at cell centres and exactly on cell borders.  Needs the built
library and no device."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import grid_shift_ref as R

I32_MAX, I32_MIN = R.I32_MAX, R.I32_MIN
DYADIC = dict(resolution=0.25, origin_x=-37.5, origin_y=-37.5, width=97, height=61)
TENTH = dict(resolution=np.float32(0.1), origin_x=np.float32(-12.3), origin_y=np.float32(4.7), width=200, height=33)
SHIFTS = [0, 1, -1, 3, -3, 64, -64, 8191, -8191, I32_MIN, I32_MAX]
FLT_MAX = float(np.finfo(np.float32).max)
EDGE = dict(resolution=2.0 ** 102, origin_x=FLT_MAX, origin_y=-FLT_MAX, width=8, height=8)   # a cell is a quarter of an ulp of FLT_MAX
EDGE_CASES = [(1, -1, R.OK), (1, 0, R.OK), (0, -1, R.OK), (-1, 1, R.OK), (-4, 4, R.OK), (2, 0, R.ERR_RANGE), (0, -2, R.ERR_RANGE),
              (3, -1, R.ERR_RANGE), (1, -3, R.ERR_RANGE)]


def c_geo(lom, g):
    return lom.capi.OccupancyGeometry(float(g["resolution"]), float(g["origin_x"]), float(g["origin_y"]), int(g["width"]), int(g["height"]))


def bits_of(c):
    return R.geometry_bits(dict(resolution=c.resolution, origin_x=c.origin_x, origin_y=c.origin_y, width=c.width, height=c.height))


@pytest.mark.parametrize("geo", [DYADIC, TENTH], ids=["dyadic", "tenth"])
def test_shift_geometry_bits(lom, geo):
    L = lom.capi.lib()
    for dx in SHIFTS:
        for dy in SHIFTS:
            out = lom.capi.OccupancyGeometry()
            status, want = R.shift_geometry(geo, dx, dy)
            assert status == R.OK
            assert L.lom_grid_shift_geometry(C.byref(c_geo(lom, geo)), dx, dy, C.byref(out)) == R.OK
            assert bits_of(out) == R.geometry_bits(want), (dx, dy)
            assert bits_of(lom.grid_shift_geometry(geo, dx, dy)) == R.geometry_bits(want)     # the module function, from a dict
    # a dyadic geometry is exact: out and back returns the bits, and the origin is the f64 value
    there = lom.grid_shift_geometry(DYADIC, 8191, -64)
    assert there.origin_x == -37.5 + 8191 * 0.25 and there.origin_y == -37.5 - 16.0
    assert bits_of(lom.grid_shift_geometry(there, -8191, 64)) == R.geometry_bits(DYADIC)
    # r = 0.1f: a shift by one cell moves the origin by one cell to under an ulp of the origin
    one = lom.grid_shift_geometry(TENTH, 1, 0)
    exact = float(TENTH["origin_x"]) + float(TENTH["resolution"])
    assert abs(float(one.origin_x) - exact) < float(np.spacing(np.float32(abs(exact))))
    # in place
    g = c_geo(lom, DYADIC)
    assert L.lom_grid_shift_geometry(C.byref(g), 3, -3, C.byref(g)) == R.OK
    assert bits_of(g) == R.geometry_bits(R.shift_geometry(DYADIC, 3, -3)[1])


def test_shift_geometry_refusals(lom):
    L = lom.capi.lib()
    big = dict(resolution=1e30, origin_x=3e38, origin_y=0.0, width=8, height=8)
    sentinel = lom.capi.OccupancyGeometry(7.0, 8.0, 9.0, 10, 11)
    before = bytes(sentinel)
    for dx, dy in ((1000000000, 0), (I32_MAX, 0), (0, I32_MAX), (0, I32_MIN)):
        big_y = dict(big, origin_x=0.0, origin_y=3e38 if dy > 0 else -3e38) if dy else big
        assert R.shift_geometry(big_y, dx, dy)[0] == R.ERR_RANGE
        assert L.lom_grid_shift_geometry(C.byref(c_geo(lom, big_y)), dx, dy, C.byref(sentinel)) == R.ERR_RANGE
        assert bytes(sentinel) == before                                                         # out untouched
    assert L.lom_grid_shift_geometry(C.byref(c_geo(lom, big)), -100000000, 0, C.byref(sentinel)) == R.OK    # towards zero: finite
    sentinel = lom.capi.OccupancyGeometry(7.0, 8.0, 9.0, 10, 11)
    # at the very edge of f32: a quarter of an ulp beyond FLT_MAX rounds back to FLT_MAX, half an ulp is a tie that goes to 2^128
    for dx, dy, status in EDGE_CASES:
        assert R.shift_geometry(EDGE, dx, dy)[0] == status
        out = lom.capi.OccupancyGeometry(7.0, 8.0, 9.0, 10, 11)
        assert L.lom_grid_shift_geometry(C.byref(c_geo(lom, EDGE)), dx, dy, C.byref(out)) == status, (dx, dy)
        assert bits_of(out) == R.geometry_bits(R.shift_geometry(EDGE, dx, dy)[1]) if status == R.OK else bytes(out) == before
    assert lom.grid_shift_geometry(EDGE, 1, -1).origin_x == FLT_MAX and lom.grid_shift_geometry(EDGE, 1, -1).origin_y == -FLT_MAX
    with pytest.raises(lom.LomError) as e:
        lom.grid_shift_geometry(big, I32_MAX, 0)
    assert e.value.code == R.ERR_RANGE
    nan, inf = math.nan, math.inf
    bad = [dict(DYADIC, resolution=0.0), dict(DYADIC, resolution=-0.25), dict(DYADIC, resolution=nan), dict(DYADIC, resolution=inf),
           dict(DYADIC, origin_x=nan), dict(DYADIC, origin_y=-inf), dict(DYADIC, width=0), dict(DYADIC, height=0),
           dict(DYADIC, width=16385), dict(DYADIC, height=16385)]
    for g in bad:
        assert R.shift_geometry(g, 1, 1)[0] == R.ERR_ARG
        assert L.lom_grid_shift_geometry(C.byref(c_geo(lom, g)), 1, 1, C.byref(sentinel)) == R.ERR_ARG, g
        assert bytes(sentinel) == before
    assert L.lom_grid_shift_geometry(C.byref(c_geo(lom, dict(DYADIC, width=16384, height=16384))), 1, 1, C.byref(sentinel)) == R.OK
    assert L.lom_grid_shift_geometry(None, 1, 1, C.byref(sentinel)) == R.ERR_ARG
    assert L.lom_grid_shift_geometry(C.byref(c_geo(lom, DYADIC)), 1, 1, None) == R.ERR_ARG


def test_symbols_are_declared_exported_and_bound(lom):
    """the two rule functions are declared with their parameters; the seven shifts through function types, one per family"""
    import os
    import re

    from tests.conftest import ROOT

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read(), flags=re.S)
    L = lom.capi.lib()
    for name in ("lom_grid_shift_geometry", "lom_grid_follow"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in lom.capi.EXPORTED and hasattr(L, name)
    families = ("occupancy", "elevation", "clearance", "navfield", "regions", "visibility", "rollout")
    assert lom.capi.EXPORTED_BY_TYPE_SHIFT == ["lom_%s_shift" % f for f in families]
    for f in families:
        name = "lom_%s_shift" % f
        assert re.search(r"typedef int\(%s_fn\)\(lom_%s \*\w+, int32_t dx, int32_t dy\);" % (name, f), hdr), name
        assert re.search(r"\b%s_fn %s;" % (name, name), hdr), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_int32, C.c_int32]
    assert re.search(r"#define LOM_ABI_VERSION 2\b", hdr) and L.lom_abi_version() == 2
    for cls in ("OccupancyGrid", "ElevationGrid", "ClearanceGrid", "NavField", "RegionGrid", "VisibilityGrid", "RolloutGrid"):
        assert callable(getattr(getattr(lom, cls), "shift"))


def admissible(n):
    """every (margin, quantum) with margin + quantum <= n / 2 and quantum >= 1"""
    return [(m, qu) for qu in range(1, n // 2 + 1) for m in range(0, n // 2 - qu + 1)]


def test_follow_exhaustive(lom):
    """x walks the cells at their centres, y walks them in reverse exactly on their lower borders (dyadic: origin + q r is
    exact); with r = 0.1f both walk centres.  One call answers both axes."""
    L = lom.capi.lib()
    fn = L.lom_grid_follow
    q = np.arange(-200, 240, dtype=np.int64)
    qr = q[::-1].copy()
    dx, dy = C.c_int32(), C.c_int32()
    pdx, pdy = C.byref(dx), C.byref(dy)
    n_calls = n_moved = n_negative = 0
    for name, r, o in (("dyadic", 0.25, -37.5), ("tenth", float(np.float32(0.1)), float(np.float32(-12.3)))):
        xs = (o + (q.astype(np.float64) + 0.5) * r).tolist()
        ys = ((o + qr.astype(np.float64) * r) if name == "dyadic" else (o + (qr.astype(np.float64) + 0.5) * r)).tolist()
        for k in range(len(q)):   # the placements mean what they should: the restated index rule gives q back
            assert R.cell_of(xs[k], o, r) == q[k] and R.cell_of(ys[k], o, r) == qr[k], (name, k)
        for n in range(2, 41):
            g = lom.capi.OccupancyGeometry(r, o, o, n, n)
            pg = C.byref(g)
            for margin, quantum in admissible(n):
                got = np.empty((len(q), 2), np.int64)
                for k in range(len(q)):
                    rc = fn(pg, xs[k], ys[k], margin, quantum, pdx, pdy)
                    assert rc == 0
                    got[k, 0], got[k, 1] = dx.value, dy.value
                n_calls += len(q)
                for axis, cells in ((0, q), (1, qr)):
                    d = got[:, axis]
                    assert np.array_equal(d, R.follow_cells(cells, n, margin, quantum)), (name, n, margin, quantum, axis)
                    after = cells - d                                 # the robot's cell in the shifted grid
                    assert ((after >= margin) & (after < n - margin)).all(), (name, n, margin, quantum, axis)
                    assert (d % quantum == 0).all()
                    inside = (cells >= margin) & (cells < n - margin)
                    assert (d[inside] == 0).all() and (d[~inside] != 0).all()
                    n_moved += int((d != 0).sum())
                    n_negative += int((d < 0).sum())
    assert n_calls == 2 * 2870 * 440 and n_moved > n_calls and n_negative > n_calls // 4


def test_follow_truncates_towards_zero_and_matches_the_scalar_rule(lom):
    g = dict(resolution=0.25, origin_x=-37.5, origin_y=10.0, width=20, height=12)
    # n = 20, n / 2 = 10, quantum 4: q = -1 -> (-11) / 4 -> -2 (not -3) -> d = -8; q = 21 -> 11 / 4 -> 2 -> d = 8
    for q, want in ((-1, -8), (-2, -12), (-5, -12), (-6, -16), (21, 8), (22, 12), (25, 12), (26, 16), (3, 0), (0, 0), (19, 0)):
        x = -37.5 + (q + 0.5) * 0.25
        assert lom.grid_follow(g, x, 10.0 + 5.5 * 0.25, 0, 4) == (want, 0), q
        assert R.follow(g, x, 10.0 + 5.5 * 0.25, 0, 4) == (R.OK, want, 0)
    # odd sides: n / 2 is the integer division
    g = dict(g, width=21, height=13)
    assert lom.grid_follow(g, -37.5 + 21.5 * 0.25, 10.0 - 0.5 * 0.25, 2, 1) == (11, -7)
    rng = np.random.default_rng(5)
    for _ in range(2000):
        n, h = int(rng.integers(2, 300)), int(rng.integers(2, 300))
        quantum = int(rng.integers(1, min(n, h) // 2 + 1))
        margin = int(rng.integers(0, min(n, h) // 2 - quantum + 1))
        gg = dict(resolution=np.float32(rng.choice([0.1, 0.25, 0.05, 1.0])), origin_x=np.float32(rng.uniform(-500, 500)),
                  origin_y=np.float32(rng.uniform(-500, 500)), width=n, height=h)
        x, y = float(rng.uniform(-3000, 3000)), float(rng.uniform(-3000, 3000))
        status, dx, dy = R.follow(gg, x, y, margin, quantum)
        assert status == R.OK and lom.grid_follow(gg, x, y, margin, quantum) == (dx, dy)


def test_follow_refusals(lom):
    L = lom.capi.lib()
    g = dict(resolution=0.25, origin_x=-37.5, origin_y=-37.5, width=20, height=12)
    dx, dy = C.c_int32(77), C.c_int32(77)

    def call(geo, x, y, margin, quantum):
        dx.value = dy.value = 77
        rc = L.lom_grid_follow(C.byref(c_geo(lom, geo)), x, y, margin, quantum, C.byref(dx), C.byref(dy))
        assert rc == R.follow(geo, x, y, margin, quantum)[0]
        if rc != 0:
            assert (dx.value, dy.value) == (0, 0)                    # on an error both are zero
        return rc

    assert call(g, 0.0, 0.0, 2, 4) == R.OK                           # 2 + 4 <= 12 / 2
    assert call(g, 0.0, 0.0, 3, 4) == R.ERR_ARG                      # ... the height's half is 6
    assert call(dict(g, height=20), 0.0, 0.0, 6, 4) == R.OK and call(dict(g, height=20), 0.0, 0.0, 7, 4) == R.ERR_ARG
    assert call(g, 0.0, 0.0, 0, 0) == R.ERR_ARG                      # quantum == 0
    assert call(g, 0.0, 0.0, 0xFFFFFFFF, 1) == R.ERR_ARG and call(g, 0.0, 0.0, 1, 0xFFFFFFFF) == R.ERR_ARG   # no wrap of the sum
    assert call(dict(g, width=1), 0.0, 0.0, 0, 1) == R.ERR_ARG       # a side of one cell has no admissible pair
    for x, y in ((math.nan, 0.0), (0.0, math.nan), (math.inf, 0.0), (0.0, -math.inf)):
        assert call(g, x, y, 1, 1) == R.ERR_ARG
    for bad in (dict(g, resolution=0.0), dict(g, origin_x=math.nan), dict(g, width=0), dict(g, height=16385)):
        assert call(bad, 0.0, 0.0, 1, 1) == R.ERR_ARG
    assert L.lom_grid_follow(None, 0.0, 0.0, 1, 1, C.byref(dx), C.byref(dy)) == R.ERR_ARG
    assert L.lom_grid_follow(C.byref(c_geo(lom, g)), 0.0, 0.0, 1, 1, None, C.byref(dy)) == R.ERR_ARG and dy.value == 0
    assert L.lom_grid_follow(C.byref(c_geo(lom, g)), 0.0, 0.0, 1, 1, C.byref(dx), None) == R.ERR_ARG and dx.value == 0
    # |q| > 2^40: x = origin + (2^40 + 1) r is just beyond, origin + 2^40 r just inside (then |d| > INT32_MAX refuses)
    far = -37.5 + (2.0 ** 40 + 1) * 0.25
    assert call(g, far, 0.0, 1, 1) == R.ERR_RANGE and call(g, 0.0, -far, 1, 1) == R.ERR_RANGE
    assert call(g, -37.5 + 2.0 ** 40 * 0.25, 0.0, 1, 1) == R.ERR_RANGE
    assert call(g, 1e308, 0.0, 1, 1) == R.ERR_RANGE
    # |d| <= INT32_MAX is the last shift that is given: q - n / 2 = 2^31 - 1 with quantum 1, and one cell further
    edge = -37.5 + (I32_MAX + 10 + 0.5) * 0.25
    assert call(g, edge, -37.0, 1, 1) == R.OK and dx.value == I32_MAX
    assert call(g, edge + 0.25, -37.0, 1, 1) == R.ERR_RANGE
    assert call(g, -37.5 + (-I32_MAX + 10 + 0.5) * 0.25, -37.0, 1, 1) == R.OK and dx.value == -I32_MAX
    assert call(g, -37.5 + (-I32_MAX + 9 + 0.5) * 0.25, -37.0, 1, 1) == R.ERR_RANGE
    with pytest.raises(lom.LomError) as e:
        lom.grid_follow(g, far, 0.0, 1, 1)
    assert e.value.code == R.ERR_RANGE
