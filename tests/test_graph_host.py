"""The pose graph without a GPU: the numpy reference's own properties (tests/graph_ref.py: Jacobians against central
differences, its LM reaching gtol on every graph tests/test_graph_gpu.py uses, inside the caps that test passes), the
stateless host functions (gauge check, LM policy step, information from a quality report), the ABI, and every refusal that
comes before device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import graph_cases as gc
from tests import graph_ref as ref
from tests.conftest import ROOT


def test_reference_jacobians_against_central_differences():
    rng = np.random.default_rng(0)
    worst, h = 0.0, 1e-6
    angles = [0.0, 1e-10, 1e-5, 0.3, 1.7, 2.9, 3.0]  # the series branch of Jl^-1, and errors near 3 rad
    for trial in range(21):
        Xi, Xj = (np.concatenate([5 * rng.normal(size=3), ref.quat_exp(rng.normal(size=3))]) for _ in range(2))
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        off = np.concatenate([0.1 * rng.normal(size=3), ref.quat_exp(axis * angles[trial % len(angles)])])
        Z = ref.compose(ref.between(Xi, Xj), off)
        th = np.linalg.norm(ref.error(Xi, Xj, Z)[:3])
        assert abs(th - angles[trial % len(angles)]) < 1e-9
        X = [Xi, Xj]
        for which, A in enumerate(ref.jacobians(Xi, Xj, Z)):
            num = np.zeros((6, 6))
            for k in range(6):
                d = np.zeros((1, 6))
                d[0, k] = h
                Xp, Xm = list(X), list(X)
                Xp[which] = ref.retract(X[which][None], d, [False])[0]
                Xm[which] = ref.retract(X[which][None], -d, [False])[0]
                num[:, k] = (ref.error(Xp[0], Xp[1], Z) - ref.error(Xm[0], Xm[1], Z)) / (2 * h)
            worst = max(worst, float(np.abs(num - A).max()))
    print("largest difference:", worst)
    assert worst < 1e-7


@pytest.mark.parametrize("name", gc.CASES + ("n65_exact",))
def test_reference_lm_meets_the_conditions_of_the_gpu_tests(name):
    poses, st = gc.optimum(name, count_pcg=True)
    print(name, {k: st[k] for k in ("outer", "accepted", "pcg_iters", "cost_initial", "cost_final", "grad_max")})
    assert st["stop_reason"] == ref.STOP_GRADIENT and st["grad_max"] <= gc.PARAMS["gtol"]
    assert st["outer"] <= 12 and st["pcg_capped"] == 0 and max(st["pcg_iters"]) <= 60  # caps passed: 30 and 200
    lin = ref.linearise(gc.case(name)[0], poses)
    assert st["cost_final"] == lin["cost"]
    if name == "n600_hubs":
        deg = np.bincount(gc.case(name)[0]["ij"].reshape(-1))
        assert deg[0] >= 200 and deg[300] >= 190 and not gc.case(name)[0]["fixed"][300]


def test_matvec_of_the_reference_is_the_dense_product():
    graph, _ = gc.case("n7_duplicates")
    lin = ref.linearise(graph, None, 0.5)
    H, free = ref.dense_system(graph, lin)
    p = np.random.default_rng(1).normal(size=(7, 6))
    y, y_abs = ref.matvec(graph, lin, 0.5, p)
    pf = np.where(np.asarray(graph["fixed"])[:, None], 0.0, p).reshape(-1)
    want = (H + 0.5 * np.diag(np.diag(H))) @ pf
    want[:6] = 0.0
    assert np.abs(y.reshape(-1) - want).max() <= 1e-12 * y_abs.max()
    blocks = np.stack([H[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(1, 7)])
    assert np.abs(lin["hdiag"][1:] - blocks - 0.5 * np.einsum("kab,ab->kab", blocks, np.eye(6))).max() <= 1e-9


# ---- stateless host functions ------------------------------------------------------------------------------------------
def _gauge(lom, fixed, ij):
    f = np.ascontiguousarray(fixed, np.int32)
    e = np.ascontiguousarray(ij, np.int32).reshape(-1, 2)
    bad = C.c_int64(-7)
    rc = lom.capi.lib().lom_graph_check_gauge(len(f), f.ctypes.data, len(e), e.ctypes.data, C.byref(bad))
    return rc, bad.value


def test_gauge_check(lom):
    E = lom.capi.ERR_ARG
    assert _gauge(lom, [1, 0, 0], [(0, 1), (1, 2)]) == (0, -1)
    assert _gauge(lom, [1, 0, 0], [(0, 1)]) == (E, 2)                    # a free isolated node
    assert _gauge(lom, [1, 0, 0, 0, 0], [(0, 1), (3, 4), (2, 3)]) == (E, 2)  # a free component
    assert _gauge(lom, [1, 1, 1], []) == (0, -1)                          # fixed only
    assert _gauge(lom, [1, 1], [(0, 1)]) == (0, -1)
    assert _gauge(lom, [], []) == (0, -1)
    assert _gauge(lom, [1, 0], [(1, 1)]) == (E, -1)                       # i == j
    assert _gauge(lom, [1, 0], [(0, 2)]) == (E, -1) and _gauge(lom, [1, 0], [(-1, 0)]) == (E, -1)
    assert _gauge(lom, [0, 0, 1], [(0, 1), (1, 2)]) == (0, -1)
    L = lom.capi.lib()
    assert L.lom_graph_check_gauge(2, None, 0, None, None) == E and L.lom_graph_check_gauge(-1, None, 0, None, None) == E


def test_policy_step_bit_for_bit(lom):
    L = lom.capi.lib()
    cases = [(10.0, 4.0, 12.0, 1e-3, 2.0), (10.0, 9.99, 12.0, 1e-3, 8.0), (10.0, 1.0, 18.1, 0.7, 2.0),  # accept: 1/3 floor, middle
             (10.0, 5.0, 10.0, 2.0, 4.0), (10.0, 10.0, 3.0, 1.0, 2.0), (10.0, 11.0, 3.0, 1.0, 16.0),  # rho = 1; reject: 0, < 0
             (10.0, float("nan"), 3.0, 1.0, 2.0), (10.0, 5.0, 0.0, 1.0, 2.0), (10.0, 12.0, 0.0, 1.0, 2.0),
             (10.0, 10.0, 0.0, 1.0, 2.0), (10.0, 5.0, -3.0, 1.0, 2.0), (1e300, -1e300, 1.0, 1.0, 2.0)]
    for cost, cost_new, denom, lam, nu in cases:
        want = ref.lm_policy(cost, cost_new, denom, lam, nu)
        l, v, r = C.c_double(lam), C.c_double(nu), C.c_double()
        got = L.lom_graph_lm_policy(cost, cost_new, denom, C.byref(l), C.byref(v), C.byref(r))
        assert bool(got) == want[0]
        assert np.float64(l.value).tobytes() == np.float64(want[1]).tobytes(), (cost, cost_new, denom)
        assert v.value == want[2]
        assert np.float64(r.value).tobytes() == np.float64(want[3]).tobytes() or (np.isnan(r.value) and np.isnan(want[3]))
    assert L.lom_graph_lm_policy(1.0, 0.5, 1.0, None, None, None) == lom.capi.ERR_ARG


def test_information_from_quality(lom):
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    H = A @ A.T + np.eye(6)
    rep = lom.capi.QualityReport()
    rep.valid = 7
    rep.information[:] = list(H.reshape(-1))
    S = np.diag([0.5, 0.5, 0.5, 1, 1, 1])
    P = np.diag([0, 0, 0, 100.0, 100, 100])
    assert np.array_equal(lom.graph_information_from_quality(rep, False), S @ H @ S)
    assert np.array_equal(lom.graph_information_from_quality(rep, True), S @ (H + P) @ S)
    rep.valid = 6
    with pytest.raises(lom.LomError) as e:
        lom.graph_information_from_quality(rep, True)
    assert e.value.code == lom.capi.ERR_ARG
    out = np.zeros(36)
    L = lom.capi.lib()
    assert L.lom_graph_information_from_quality(None, 1, out.ctypes.data) == lom.capi.ERR_ARG
    assert L.lom_graph_information_from_quality(C.byref(rep), 1, None) == lom.capi.ERR_ARG


def test_pose_conversions(lom):
    L = lom.capi.lib()
    p32 = lom.capi.Pose(lom.capi.f3((1.5, -2.25, 0.1)), lom.capi.f4((0.5, 0.5, -0.5, 0.5)))
    p64 = np.zeros(1, lom.capi.GRAPH_POSE)
    assert L.lom_graph_pose_from_f32(C.byref(p32), p64.ctypes.data) == 0
    assert p64["t"][0].tolist() == [1.5, -2.25, float(np.float32(0.1))] and p64["q_wxyz"][0].tolist() == [0.5, 0.5, -0.5, 0.5]
    back = lom.capi.Pose()
    assert L.lom_graph_pose_to_f32(p64.ctypes.data, C.byref(back)) == 0
    assert bytes(back) == bytes(p32)
    assert L.lom_graph_pose_from_f32(None, p64.ctypes.data) == lom.capi.ERR_ARG
    assert L.lom_graph_pose_to_f32(p64.ctypes.data, None) == lom.capi.ERR_ARG


# ---- ABI -------------------------------------------------------------------------------------------------------------
GRAPH_SYMBOLS = ["lom_graph_create", "lom_graph_destroy", "lom_graph_last_error", "lom_graph_clear", "lom_graph_stream",
                 "lom_graph_device", "lom_graph_add_node", "lom_graph_add_nodes", "lom_graph_add_edge", "lom_graph_add_edges",
                 "lom_graph_node_count", "lom_graph_edge_count", "lom_graph_get_poses", "lom_graph_set_pose",
                 "lom_graph_set_fixed", "lom_graph_optimize", "lom_graph_evaluate", "lom_graph_debug_matvec",
                 "lom_graph_edge_chi2", "lom_graph_check_gauge", "lom_graph_lm_policy", "lom_graph_information_from_quality",
                 "lom_graph_pose_from_f32", "lom_graph_pose_to_f32"]


def test_symbols_declared_exported_and_sized(lom):
    hdr = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    assert re.search(r"#define LOM_ABI_VERSION 2\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = lom.capi.lib()
    assert sorted(set(re.findall(r"\b(lom_graph_[a-z0-9_]+)\s*\(", code))) == sorted(GRAPH_SYMBOLS)
    for name in GRAPH_SYMBOLS:
        assert name in lom.capi.EXPORTED and hasattr(L, name), name
    assert lom.capi.GRAPH_POSE.itemsize == 56 and C.sizeof(lom.capi.GraphParams) == 40 and C.sizeof(lom.capi.GraphStats) == 56
    assert lom.capi.GraphStats.cost_initial.offset == 24
    assert L.lom_abi_version() == 2


def test_null_and_bad_arguments_are_refused_without_a_device(lom):
    L, E = lom.capi.lib(), lom.capi.ERR_ARG
    h = C.c_void_p()
    assert L.lom_graph_create(0, 4, 4, None) == E
    assert L.lom_graph_create(0, 1 << 28, 4, C.byref(h)) == E and not h.value
    assert L.lom_graph_create(0, 4, 1 << 28, C.byref(h)) == E and not h.value
    pose = np.zeros(1, lom.capi.GRAPH_POSE)
    pose["q_wxyz"][0, 0] = 1.0
    om, d, f, ij = np.eye(6), np.zeros(1), np.zeros(1, np.int32), np.array([[0, 1]], np.int32)
    out = np.zeros(36)
    prm, st = lom.capi.GraphParams(1e-4, 1e-5, 1e-12, 1e-8, 10, 10), lom.capi.GraphStats()
    assert L.lom_graph_clear(None) == E and L.lom_graph_device(None) == E and L.lom_graph_stream(None) is None
    assert L.lom_graph_add_node(None, pose.ctypes.data, 0) == E
    assert L.lom_graph_add_nodes(None, pose.ctypes.data, f.ctypes.data, 1) == E
    assert L.lom_graph_add_edge(None, 0, 1, pose.ctypes.data, om.ctypes.data, 0.0) == E
    assert L.lom_graph_add_edges(None, ij.ctypes.data, pose.ctypes.data, om.ctypes.data, d.ctypes.data, 1) == E
    assert L.lom_graph_node_count(None) == E and L.lom_graph_edge_count(None) == E
    assert L.lom_graph_get_poses(None, 0, 1, pose.ctypes.data) == E
    assert L.lom_graph_set_pose(None, 0, pose.ctypes.data) == E and L.lom_graph_set_fixed(None, 0, 1) == E
    assert L.lom_graph_optimize(None, C.byref(prm), C.byref(st)) == E
    assert L.lom_graph_evaluate(None, 0.0, None, None, None, None, None) == E
    assert L.lom_graph_debug_matvec(None, 0.0, out.ctypes.data, out.ctypes.data) == E
    assert L.lom_graph_edge_chi2(None, 0, 1, out.ctypes.data) == E
    L.lom_graph_destroy(None)
    assert L.lom_graph_last_error(None) is not None
    if L.lom_device_count() < 1:  # a host without a device: a loud failure, no fallback
        with pytest.raises(lom.LomError) as e:
            lom.PoseGraph()
        assert e.value.code == lom.capi.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(TypeError):
        lom.graphParams(dict(lambda0=1.0))
