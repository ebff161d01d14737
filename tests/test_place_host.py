"""Place recognition without a GPU: the numpy reference's own properties (tests/place_ref.py), the conditions every
scene set must meet before tests/test_place_gpu.py asks the device about it, the ABI (symbols, struct sizes, version),
and the refusals of every bad argument, which come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import place_ref as ref
from tests.conftest import ROOT

P, PB = ref.PARAMS, ref.PARAMS_BIG


@pytest.mark.parametrize("seed", range(1, 13))
def test_scene_clouds_have_no_ill_point(seed):
    for params in (P, PB):
        xyz = ref.scene_cloud(seed, params)
        desc, ill = ref.describe(xyz, params)
        assert not ill.any()
        assert (desc > 0).sum() > desc.size // 3
        r = np.hypot(xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64))
        assert (r > params[2]).any() and (xyz[:, 2] <= np.float32(params[3])).any()  # ignored points are present


def test_query_sets_meet_the_conditions():
    """no skip: a set that does not meet the conditions fails here (and the GPU test asserts the same)"""
    for params, n, sizes, sub in ((P, 1000, ref.QUERY_SIZES, ref.SUB_RANGE), (PB, 65, (9, 65), (3, 40))):
        qs, entries, bad = ref.query_set(params, n, sizes, sub)
        assert bad == [] and len(entries) == n
        ranges = [(0, s) for s in sizes] + [sub]
        assert ref.check_conditions(qs, entries, params, 64, ranges) == []
        ids, dist, shift, _ = ref.query(qs, entries, 5)
        S = params[1]
        assert ids[0, 0] == 0 and shift[0, 0] == S - 11 and ids[1, 0] == 1 and shift[1, 0] == S - 29  # columns moved by +11, +29


def test_sign_scene_meets_the_conditions():
    a, _ = ref.describe(ref.scene_cloud(3, P), P)
    b, _ = ref.describe(ref.scene_cloud(3, P, rotate_sectors=7), P)
    assert ref.check_conditions([b], a[None], P, 1, [(0, 1)]) == []


@pytest.mark.parametrize("k", [0, 1, 7, 59])
def test_rotation_by_k_sectors(k):
    R, S = P[:2]
    a, _ = ref.describe(ref.scene_cloud(5, P), P)
    b, ill = ref.describe(ref.scene_cloud(5, P, rotate_sectors=k), P)
    assert not ill.any()
    d = ref.distances(b, a)
    assert int(np.argmin(d)) == (S - k) % S and d.min() < ref.tol(R, S)
    assert np.array_equal(b, np.roll(a, k, axis=1))


def test_duplicates_rank_by_id_and_padding():
    e = ref.scene_descriptor(4, P)
    entries = np.stack([ref.scene_descriptor(5, P), e, e, ref.scene_descriptor(6, P)])
    ids, dist, shift, alld = ref.query(e, entries, 6)
    assert ids[0].tolist() == [1, 2] + ids[0, 2:4].tolist() + [-1, -1] and dist[0, 0] == dist[0, 1] < 1e-12
    assert np.isinf(dist[0, 4:]).all() and (shift[0, 4:] == 0).all()
    ids, dist, _, _ = ref.query(e, entries, 3, 2, 2)
    assert (ids == -1).all() and np.isinf(dist).all()


def test_equal_columns_tie_at_shift_zero_and_zero_descriptor():
    R, S = P[:2]
    col = np.linspace(0.5, 2.0, R, dtype=np.float32)
    same = np.repeat(col[:, None], S, axis=1)
    d = ref.distances(same, same)
    assert np.all(d == d[0]) and int(np.argmin(d)) == 0
    zero = np.zeros((R, S), np.float32)
    assert np.all(ref.distances(zero, same) == 1.0) and np.all(ref.distances(same, zero) == 1.0)
    assert ref.describe(np.zeros((0, 3), np.float32), P)[0].tobytes() == zero.tobytes()
    with pytest.raises(ValueError):
        ref.describe(np.array([[1, np.nan, 0]], np.float32), P)


def test_f32_sum_order_stays_within_the_tolerance():
    """The device's arithmetic restated in numpy f32 -- unit columns rounded to f32, per entry column a chain over the
    rings from 0, then the columns in order, one division, max(d, 0) -- against the f64 reference on the GPU test's own
    scenes: within TOL, every shift equal.  (numpy has no fused multiply-add; the device's chain rounds once per term
    instead of twice, which the derivation's R u per dot product covers either way.)"""
    R, S = P[:2]
    qs, entries, _ = ref.query_set()
    n = 120

    def unit32(d):
        d64 = d.astype(np.float64)
        nrm = np.sqrt((d64 * d64).sum(axis=-2, keepdims=True))
        nz = nrm > 0
        return np.where(nz, d64 / np.where(nz, nrm, 1), 0).astype(np.float32), nz.squeeze(-2)

    cu, cm = unit32(entries[:n])
    for q in qs:
        qu, qm = unit32(q)
        want = ref.distances_many(q, entries[:n])
        got = np.ones((n, S), np.float32)
        for s in range(S):
            tot = np.zeros(n, np.float32)
            for jc in range(S):
                dot = np.zeros(n, np.float32)
                for r in range(R):
                    dot = dot + qu[r, (jc - s) % S] * cu[:, r, jc]
                tot = tot + dot
            cnt = (qm[None, :] & np.roll(cm, -s, axis=1)).sum(axis=1)
            d = np.maximum(np.float32(1) - tot / np.maximum(cnt, 1).astype(np.float32), np.float32(0))
            got[:, s] = np.where(cnt > 0, d, np.float32(1))
        assert got.dtype == np.float32 and np.abs(got - want).max() <= ref.tol(R, S)
        assert np.array_equal(got.argmin(axis=1), want.argmin(axis=1))


def test_tolerance_value():
    assert abs(ref.tol(20, 60) - 6.6e-6) < 1e-7


# ---- ABI ----------------------------------------------------------------------------------------------------------

PLACE_SYMBOLS = ["lom_place_db_create", "lom_place_db_destroy", "lom_place_db_last_error", "lom_place_db_size",
                 "lom_place_db_clear", "lom_place_db_params", "lom_place_describe", "lom_place_describe_device",
                 "lom_place_db_add", "lom_place_db_add_cloud", "lom_place_db_add_cloud_device", "lom_place_db_get",
                 "lom_place_db_query", "lom_place_db_query_cloud_device", "lom_place_shift_yaw",
                 "lom_odometry_place_descriptor",
                 # beyond the issue's list: what the odometry entry needs to order and place its read
                 "lom_place_db_stream", "lom_place_db_device", "lom_place_db_wait_event", "lom_frontend_deskewed"]


def test_symbols_declared_exported_and_sized(lom):
    hdr = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    assert re.search(r"#define LOM_ABI_VERSION 2\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = lom.capi.lib()
    for name in PLACE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in lom.capi.EXPORTED and hasattr(L, name), name
    assert C.sizeof(lom.capi.PlaceParams) == 16 and lom.capi.PLACE_MATCH.itemsize == 16
    assert L.lom_abi_version() == 2


def _pp(lom, rings=20, sectors=60, max_range=80.0, z_floor=-1.5):
    return lom.capi.PlaceParams(rings, sectors, max_range, z_floor)


BAD_PARAMS = [dict(rings=0), dict(rings=65), dict(sectors=0), dict(sectors=65), dict(max_range=float("nan")),
              dict(max_range=float("inf")), dict(max_range=0.0), dict(max_range=-1.0), dict(z_floor=float("nan")),
              dict(z_floor=float("inf"))]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_bad_params_are_refused_without_a_device(lom, bad):
    L, E = lom.capi.lib(), lom.capi.ERR_ARG
    h = C.c_void_p()
    p = _pp(lom, **bad)
    assert L.lom_place_db_create(C.byref(p), 0, 4, C.byref(h)) == E and not h.value
    assert np.isnan(L.lom_place_shift_yaw(C.byref(p), 1))
    with pytest.raises(lom.LomError) as e:
        lom.PlaceDatabase(p)
    assert e.value.code == E


def test_null_and_invalid_arguments_are_refused_without_a_device(lom):
    L, E = lom.capi.lib(), lom.capi.ERR_ARG
    h = C.c_void_p()
    p = _pp(lom)
    assert L.lom_place_db_create(None, 0, 4, C.byref(h)) == E
    assert L.lom_place_db_create(C.byref(p), 0, 4, None) == E
    desc = np.zeros((20, 60), np.float32)
    xyz = np.zeros((4, 3), np.float32)
    out = np.zeros(64, lom.capi.PLACE_MATCH)
    assert L.lom_place_db_size(None) == E and L.lom_place_db_clear(None) == E
    assert L.lom_place_db_params(None, C.byref(p)) == E
    assert L.lom_place_describe(None, xyz.ctypes.data, 4, 12, desc.ctypes.data) == E
    assert L.lom_place_describe_device(None, xyz.ctypes.data, 4, 12, desc.ctypes.data) == E
    assert L.lom_place_db_add(None, desc.ctypes.data) == E
    assert L.lom_place_db_add_cloud(None, xyz.ctypes.data, 4, 12) == E
    assert L.lom_place_db_add_cloud_device(None, xyz.ctypes.data, 4, 12) == E
    assert L.lom_place_db_get(None, 0, desc.ctypes.data) == E
    # (a host without a device cannot create a handle, so these check the NULL refusal only; bad k, ids and descriptors
    # on a live database: tests/test_place_gpu.py::test_refusals_on_a_live_database)
    for k in (0, 65):
        assert L.lom_place_db_query(None, desc.ctypes.data, 1, 0, 0, k, out.ctypes.data, None) == E
        assert L.lom_place_db_query_cloud_device(None, xyz.ctypes.data, 4, 12, 0, 0, k, out.ctypes.data) == E
    assert L.lom_place_db_query(None, desc.ctypes.data, 1, 3, 2, 1, out.ctypes.data, None) == E
    assert L.lom_place_db_wait_event(None, None) == E and L.lom_place_db_device(None) == E
    assert L.lom_place_db_stream(None) is None
    assert L.lom_frontend_deskewed(None, None, None) == E
    assert L.lom_odometry_place_descriptor(None, None, 0, desc.ctypes.data, None) == E
    L.lom_place_db_destroy(None)
    assert L.lom_place_db_last_error(None) is not None


def test_shift_yaw(lom):
    L = lom.capi.lib()
    p = _pp(lom)
    for shift in (0, 1, 53, 59, 60, 61):
        want = ((60 - shift % 60) % 60) * 2 * np.pi / 60
        assert L.lom_place_shift_yaw(C.byref(p), shift) == want
    assert L.lom_place_shift_yaw(C.byref(p), 53) == 7 * 2 * np.pi / 60
