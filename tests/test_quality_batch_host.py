"""Host side of the batched quality report, without a GPU: the new C ABI symbols, lom_pose_lattice against a numpy
restatement written here (node count, order, and the bytes of t and q), lom_quality_batch_best's ranking, and the
argument errors of the batch entries that are rejected before a handle is looked at.

The lattice restatement follows include/lidar_odometry_amd.h word for word: per axis 2 * floor(half / step) + 1 nodes (one
where the step is <= 0 or the extent below it), offsets added in f64 and rounded once to f32, yaw node j as the left
product yaw_z(j * step) * q in f64, normalised, rounded to f32; yaw outermost, then x, y, z innermost, ascending.  cos and
sin come from `math` (the C library's, as the product's), every other operation is a correctly rounded IEEE one."""
import ctypes as C
import math

import numpy as np
import pytest

NEW_SYMBOLS = ["lom_match_quality_batch_sums", "lom_match_quality_batch_sums_device", "lom_match_quality_batch",
               "lom_match_quality_batch_device", "lom_scan_quality_batch_sums", "lom_scan_quality_batch_sums_device",
               "lom_scan_quality_batch", "lom_scan_quality_batch_device", "lom_quality_batch_best", "lom_pose_lattice"]


def test_symbols_and_constants(lom):
    L = lom.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in lom.capi.EXPORTED, name
        assert hasattr(L, name), name
    assert L.lom_abi_version() == 2
    assert lom.capi.OPT_TEST_QUALITY_ROUND_MAX == 108
    P = lom.capi.QualityProblem
    assert C.sizeof(P) == 56
    assert [(k, getattr(P, k).offset) for k, _ in P._fields_] == [("xyz", 0), ("n", 8), ("stride_bytes", 16), ("t", 24),
                                                                   ("q_wxyz", 36)]


# ---- lom_pose_lattice ----------------------------------------------------------------------------------------------

def _half_nodes(half, step):
    half, step = float(np.float32(half)), float(np.float32(step))
    if not step > 0.0 or half < step:
        return 0
    return int(math.floor(half / step))


def lattice_restated(t, q, half, step, half_yaw, step_yaw):
    """[(t f32[3], q f32[4]), ...] in the documented order"""
    t = [float(np.float32(v)) for v in t]
    cw, cx, cy, cz = [float(np.float32(v)) for v in q]
    st = [float(np.float32(v)) for v in step]
    k = [_half_nodes(half[a], step[a]) for a in range(3)]
    ky = _half_nodes(half_yaw, step_yaw)
    out = []
    for jy in range(-ky, ky + 1):
        angle = float(jy) * float(np.float32(step_yaw))
        w1, z1 = math.cos(0.5 * angle), math.sin(0.5 * angle)
        qq = [w1 * cw - z1 * cz, w1 * cx - z1 * cy, w1 * cy + z1 * cx, w1 * cz + z1 * cw]
        norm = math.sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3])
        qf = np.array([v / norm for v in qq], np.float64).astype(np.float32)
        for ix in range(-k[0], k[0] + 1):
            for iy in range(-k[1], k[1] + 1):
                for iz in range(-k[2], k[2] + 1):
                    tf = np.array([t[0] + float(ix) * st[0], t[1] + float(iy) * st[1], t[2] + float(iz) * st[2]],
                                  np.float64).astype(np.float32)
                    out.append((tf, qf))
    return out


def _lattice_raw(lom, t, q, half, step, half_yaw, step_yaw, cap=None, want_out=True):
    L = lom.capi.lib()
    c = lom.capi.Pose(lom.capi.f3(t), lom.capi.f4(q))
    n = L.lom_pose_lattice(C.byref(c), lom.capi.f3(half), lom.capi.f3(step), float(half_yaw), float(step_yaw), None, 0)
    if n < 0 or not want_out:
        return n, None
    cap = n if cap is None else cap
    out = (lom.capi.Pose * max(cap, 1))()
    C.memset(out, 0xAB, C.sizeof(out))
    n2 = L.lom_pose_lattice(C.byref(c), lom.capi.f3(half), lom.capi.f3(step), float(half_yaw), float(step_yaw), out, cap)
    assert n2 == n
    return n, out


LATTICES = [
    # the GPU test's: 3 x 3 x 1 translations, 3 yaws
    ((0.02, -0.01, 0.0), (0.99999803, 0.0, 0.0, 0.0019999987), (0.25, 0.25, 0.0), (0.25, 0.25, 0.0), math.radians(2.5),
     math.radians(2.5)),
    # uneven extents, all four axes, a tilted non-unit quaternion
    ((10.3, -7.7, 1.25), (0.99993, 0.0031, -0.0042, 0.0105), (1.0, 0.55, 0.2), (0.3, 0.25, 0.1), 0.2, 0.07),
    # an extent that is not a multiple of the step, a large translation
    ((1234.5, -987.25, 3.0), (0.70710677, 0.0, 0.70710677, 0.0), (0.99, 0.0, 0.31), (0.5, 1.0, 0.1), 0.0, 0.1),
]


@pytest.mark.parametrize("case", range(len(LATTICES)))
def test_pose_lattice_against_restatement(lom, case):
    t, q, half, step, hy, sy = LATTICES[case]
    want = lattice_restated(t, q, half, step, hy, sy)
    n, out = _lattice_raw(lom, t, q, half, step, hy, sy)
    k = [_half_nodes(half[a], step[a]) for a in range(3)] + [_half_nodes(hy, sy)]
    assert n == len(want) == (2 * k[0] + 1) * (2 * k[1] + 1) * (2 * k[2] + 1) * (2 * k[3] + 1)
    if case == 0:
        assert n == 27
    for i, (wt, wq) in enumerate(want):
        assert np.array(out[i].t[:], np.float32).tobytes() == wt.tobytes(), (i, out[i].t[:], wt)
        assert np.array(out[i].q[:], np.float32).tobytes() == wq.tobytes(), (i, out[i].q[:], wq)
    # order: z innermost and ascending, yaw outermost
    ts = np.array([o.t[:] for o in out[:n]])
    nz, ny = 2 * k[2] + 1, 2 * k[1] + 1
    if nz > 1:
        assert (np.diff(ts[:nz, 2]) > 0).all() and ts[0, 2] < float(np.float32(t[2]))
    if ny > 1:
        assert ts[nz, 1] > ts[0, 1]
    per_yaw = n // (2 * k[3] + 1)
    assert len({bytes(np.array(o.q[:], np.float32).tobytes()) for o in out[:per_yaw]}) == 1
    # the Python wrapper returns the same poses
    poses = lom.pose_lattice(lom.Pose3D(t, q), half, step, hy, sy)
    assert len(poses) == n
    assert all(p.translation.tobytes() == w[0].tobytes() and p.rotation.tobytes() == w[1].tobytes()
               for p, w in zip(poses, want))


def test_pose_lattice_degenerate_and_errors(lom):
    t, q = (1.0, 2.0, 3.0), (1.0, 0.0, 0.0, 0.0)
    # step 0, negative step, extent below the step: the centre alone
    for half, step, hy, sy in (((1, 1, 1), (0, 0, 0), 1.0, 0.0), ((1, 1, 1), (-0.5, -0.5, -0.5), 1.0, -0.1),
                               ((0.2, 0.2, 0.2), (0.25, 0.25, 0.25), 0.01, 0.02), ((0, 0, 0), (0.25, 0.25, 0.25), 0.0, 0.1)):
        n, out = _lattice_raw(lom, t, q, half, step, hy, sy)
        assert n == 1
        assert out[0].t[:] == [1.0, 2.0, 3.0] and out[0].q[:] == [1.0, 0.0, 0.0, 0.0]
    # one axis degenerate, the others not
    n, _ = _lattice_raw(lom, t, q, (0.5, 0.1, 0.5), (0.25, 0.25, 0.0), 0.0, 0.0)
    assert n == 5
    # count-only call and a cap that is too small: the count, and nothing written
    n, out = _lattice_raw(lom, t, q, (0.5, 0.5, 0.0), (0.25, 0.25, 0.25), 0.1, 0.05, cap=124)
    assert n == 125
    assert bytes(out) == b"\xAB" * C.sizeof(out)
    n, out = _lattice_raw(lom, t, q, (0.5, 0.5, 0.0), (0.25, 0.25, 0.25), 0.1, 0.05, cap=130)
    assert n == 125 and bytes(out)[125 * 28:] == b"\xAB" * (5 * 28)      # exactly n entries written
    # errors
    L = lom.capi.lib()
    h3, s3 = lom.capi.f3((1, 1, 1)), lom.capi.f3((0.5, 0.5, 0.5))
    assert L.lom_pose_lattice(None, h3, s3, 0.0, 0.0, None, 0) == lom.capi.ERR_ARG
    nan, inf = float("nan"), float("inf")
    for bad in (dict(t=(nan, 0, 0)), dict(q=(1, 0, nan, 0)), dict(q=(0, 0, 0, 0)), dict(half=(1, inf, 1)), dict(step=(0.5, 0.5, nan)),
                dict(hy=nan), dict(sy=inf)):
        a = dict(t=t, q=q, half=(1, 1, 1), step=(0.5, 0.5, 0.5), hy=0.1, sy=0.05)
        a.update(bad)
        n, _ = _lattice_raw(lom, a["t"], a["q"], a["half"], a["step"], a["hy"], a["sy"], want_out=False)
        assert n == lom.capi.ERR_ARG, bad
    with pytest.raises(lom.LomError):
        lom.pose_lattice(lom.Pose3D((nan, 0, 0)), (1, 1, 1), (0.5, 0.5, 0.5))


# ---- lom_quality_batch_best ----------------------------------------------------------------------------------------

def _reports(lom, rows):
    """rows: (queries, valid, cost)"""
    r = (lom.capi.QualityReport * max(len(rows), 1))()
    for i, (queries, valid, cost) in enumerate(rows):
        r[i].queries, r[i].valid, r[i].cost = queries, valid, cost
    return r


def test_quality_batch_best(lom):
    best = lom.capi.lib().lom_quality_batch_best
    assert best(_reports(lom, [(10, 5, 1.0), (10, 7, 9.0), (10, 6, 0.1)]), 3) == 1           # most valid
    assert best(_reports(lom, [(10, 7, 2.0), (10, 7, 1.0), (10, 7, 1.5)]), 3) == 1           # tie on valid: lower cost
    assert best(_reports(lom, [(10, 3, 2.0), (10, 7, 1.0), (10, 7, 1.0), (10, 7, 1.0)]), 4) == 1   # full tie: lower index
    # a report of no queries ranks below any other, one with zero valid included
    assert best(_reports(lom, [(0, 0, 0.0), (10, 0, 0.0), (0, 0, 0.0)]), 3) == 1
    assert best(_reports(lom, [(10, 0, 0.0), (0, 0, 0.0)]), 2) == 0
    assert best(_reports(lom, [(0, 0, 0.0), (0, 0, 0.0)]), 2) == 0
    assert best(_reports(lom, [(10, 4, 3.0)]), 1) == 0
    # only the first `count` entries are looked at
    assert best(_reports(lom, [(10, 5, 1.0), (10, 7, 9.0)]), 1) == 0
    assert best(_reports(lom, [(10, 5, 1.0)]), 0) == -1
    assert best(_reports(lom, [(10, 5, 1.0)]), -3) == -1
    assert best(None, 4) == -1


# ---- argument errors that need no device ---------------------------------------------------------------------------

def test_batch_entries_reject_a_null_handle(lom):
    L = lom.capi.lib()
    p = (lom.capi.QualityProblem * 1)()
    sums = (C.c_double * 36)(*([7.0] * 36))
    rep = (lom.capi.QualityReport * 1)()
    rep[0].queries = 77
    best = C.c_int(42)
    for name in ("lom_match_quality_batch_sums", "lom_match_quality_batch_sums_device", "lom_scan_quality_batch_sums",
                 "lom_scan_quality_batch_sums_device"):
        for count in (0, 1):
            assert getattr(L, name)(None, p, count, 0.3, sums) == lom.capi.ERR_ARG, name
    for name in ("lom_match_quality_batch", "lom_match_quality_batch_device", "lom_scan_quality_batch",
                 "lom_scan_quality_batch_device"):
        for count in (0, 1):
            assert getattr(L, name)(None, p, count, 0.3, 0.0, 0.0, rep, C.byref(best)) == lom.capi.ERR_ARG, name
    assert list(sums) == [7.0] * 36 and rep[0].queries == 77 and best.value == 42
