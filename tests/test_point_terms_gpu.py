"""The closed-form rotation columns and the branch-free Huber terms (csrc/k_eval.hpp: point_terms, huber_terms) inside
the device-resident solve: every evaluation `lom_debug_lm_trace` records, sum by sum against the oracle's
(`orc_shard_match_eval` / `orc_shard_eval_fixed`), within the bars of tests/test_eval_parity.py, whose comparison helper
is imported, on clouds whose matches sit on BOTH sides of the Huber knee at the guess.

* small_synth_case, and `knee_scene`: three mutually orthogonal planes and a scan of a few hundred points, 45 % of them
  0.2 m off their plane -- at the guess more than a third of the valid matches have |r| in (0.15, 0.3), which the test
  checks on the CPU with the oracle's pairs before it relies on it;
* the guess is an f32 pose with a rotation about a skew axis (|q|^2 - 1 of an f32 cast), and the later evaluations of a
  solve are made at f64 LM candidates whose quaternion is not unit either;
* both search modes; fewer points than one workgroup of the solve (256), and n = 1.  With ONE point the sums are held
  to the oracle's at the guess only: a solve on a single residual drives it to zero -- r falls by the LM damping, 1e-4,
  with the first step, 0.026 m -> 2.6e-6 m, and on to 1e-10 m -- while it is still the difference of coordinates of
  0.5 - 4.5 m, so every sum of the later evaluations, a product with r, carries r's rounding floor (a few 1e-16 m,
  1e-10 of r and more) whatever the code does, and the bars, relative to the sums' own scale, have no floor for that
  (with more points the cost of the others is that scale).  Measured on the first such evaluation: g[1] 1.0e-17 off
  at 4.16e-6, against a bar of 8.5e-18.  Counts, cost and pose of that align are still held to the oracle's;
* recorded iterations, evaluated points, step norm, cost and counters of the whole align equal the oracle's, the final
  pose within 1e-4 m / 1e-4 rad, as tests/test_gpu_parity.py requires.
"""
import os

import numpy as np
import pytest

from tests import scenes
from tests.test_eval_parity import _assert_lm_numbers, assert_sums_close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["product", "counted"])
def search_mode(request, monkeypatch):
    """As tests/test_gpu_parity.py: "product" handles read 0 for the reference-algorithm counts (cand, occ), "counted"
    handles (LOM_COUNT_CANDIDATES=1 at create) produce the oracle's."""
    monkeypatch.setenv("LOM_COUNT_CANDIDATES", "1" if request.param == "counted" else "0")
    return request.param


def _counted():
    return os.environ.get("LOM_COUNT_CANDIDATES") == "1"


def knee_scene(n_scan=600, seed=11):
    """Map: the planes x = 0, y = 0, z = 0, 5 x 5 m each, 8000 points per plane (a map point within 0.1 m of any
    query's foot).  Scan: points over the three planes, 55 % 0.02 m off their plane, 45 % 0.2 m off it."""
    rng = np.random.default_rng(seed)
    mp, mn = [], []
    for axis in range(3):
        uv = rng.uniform(0.0, 5.0, (8000, 2))
        pts = np.insert(uv, axis, 0.0, axis=1)
        nrm = np.zeros((len(pts), 3))
        nrm[:, axis] = 1.0
        mp.append(pts)
        mn.append(nrm)
    uv = rng.uniform(0.5, 4.5, (n_scan, 2))
    off = np.where(rng.random(n_scan) < 0.45, 0.2, 0.02)
    scan = np.empty((n_scan, 3))
    for i in range(n_scan):
        scan[i] = np.insert(uv[i], i % 3, off[i])
    return {"map_xyz": np.concatenate(mp).astype(np.float32), "map_nrm": np.concatenate(mn).astype(np.float32),
            "scan": np.ascontiguousarray(scan.astype(np.float32))}


GUESS = ((0.02, -0.015, 0.01), scenes.angle_axis_q(0.006, scenes._unit((0.3, -0.2, 1.0))))


@pytest.fixture(scope="module")
def knee():
    return knee_scene()


def _residuals_at(oracle, og, scan, guess):
    """|r| of the valid matches at the guess, from the oracle's pairs (f64)."""
    t, q = np.asarray(guess[0], np.float64), np.asarray(guess[1], np.float64)
    c = og.findMatchingPairs(scan, oracle.Pose3D(*guess), 0.3)
    ok = c["index"] >= 0
    w, u = q[0], q[1:]
    p = scan[ok].astype(np.float64)
    uv = 2.0 * np.cross(u, p)
    rp = p + w * uv + np.cross(u, uv)
    return np.abs(((rp + t - c["origin"][ok].astype(np.float64)) * c["normal"][ok].astype(np.float64)).sum(axis=1))


def _trace_vs_oracle(lom, oracle, g, og, scan, guess, outer_index, tag, later_evaluations=True):
    """tests/test_eval_parity.py's walk over a trace, for either search mode: a product handle reads 0 for the
    reference-algorithm counts, so the oracle's are zeroed before the (exact) comparison of the counters."""
    m = lom.CloudMatcher()
    pose, trace = m.debugLmTrace(g, scan, guess, outer_index)
    assert 1 <= len(trace) <= 5
    sh = oracle.Shard(og, scan)
    x0, s0 = trace[0]
    pq, pt = x0[:4].astype(np.float32), x0[4:].astype(np.float32)
    assert pq.astype(np.float64).tolist() == x0[:4].tolist() and pt.astype(np.float64).tolist() == x0[4:].tolist()
    ref = sh.match_eval(pt, pq, x0[:4], x0[4:])
    if not _counted():
        ref[29:31] = 0.0
    assert_sums_close(s0, ref, (tag, outer_index, 0))
    excess = [abs(float(x0[:4] @ x0[:4]) - 1.0)]
    for e, (x, s) in enumerate(trace[1:] if later_evaluations else [], 1):
        ref = sh.eval_fixed(x[:4], x[4:])
        ref[28:31] = s0[28:31]                 # counters travel with evaluation 0 only
        got = s.copy()
        got[28:31] = s0[28:31]
        assert_sums_close(got, ref, (tag, outer_index, e))
        excess.append(abs(float(x[:4] @ x[:4]) - 1.0))
    return pose, m.stats, len(trace), max(excess), s0


def _align_vs_oracle(lom, oracle, g, og, scan, guess, st, pose):
    om = oracle.CloudMatcher()
    ref = om.align(og, scan, oracle.Pose3D(*guess))
    ost = dict(om.stats)
    if not _counted():
        ost["cand_total"] = ost["occ_total"] = 0
    _assert_lm_numbers(st, ost)
    dt, dr = scenes.pose_delta(pose.translation, pose.rotation, ref.translation, ref.rotation)
    assert dt < 1e-4 and dr < 1e-4, (dt, dr)
    return om.stats["outer_iterations"]


def _grids(lom, oracle, case):
    g, og = lom.VoxelGrid(0.5, 20), oracle.VoxelGrid(0.5, 20)
    g.addCloud(case["map_xyz"], case["map_nrm"])
    og.addCloud(case["map_xyz"], case["map_nrm"])
    return g, og


def test_trace_across_the_huber_knee(lom, oracle, knee):
    g, og = _grids(lom, oracle, knee)
    scan = knee["scan"]
    r = _residuals_at(oracle, og, scan, GUESS)
    outliers = np.sum((r > 0.15) & (r < 0.3))
    assert len(r) > 0.9 * len(scan) and 3 * outliers >= len(r), (len(r), outliers)
    assert np.sum(r < 0.15) * 3 >= len(r)                          # ... and as many on the quadratic side
    evals, worst_excess = 0, 0.0
    for outer in (0, 1, 3):
        pose, st, ne, excess, s0 = _trace_vs_oracle(lom, oracle, g, og, scan, lom.Pose3D(*GUESS), outer, "knee")
        evals += ne
        worst_excess = max(worst_excess, excess)
        assert s0[28] == len(r) or outer > 0
    assert evals >= 6 and worst_excess > 1e-9                       # non-unit quaternions were evaluated
    _align_vs_oracle(lom, oracle, g, og, scan, GUESS, st, pose)


def test_trace_small_synth(lom, oracle):
    sm = scenes.small_synth_case()
    g, og = _grids(lom, oracle, sm)
    guess = ((0.12, -0.1, 0.03), scenes.angle_axis_q(0.008, scenes._unit((0.2, 0.1, 1.0))))
    for outer in (0, 2):
        pose, st, ne, excess, _ = _trace_vs_oracle(lom, oracle, g, og, sm["scan"], lom.Pose3D(*guess), outer, "synth")
    _align_vs_oracle(lom, oracle, g, og, sm["scan"], guess, st, pose)


@pytest.mark.parametrize("n", [1, 100])
def test_trace_fewer_points_than_a_workgroup(lom, oracle, knee, n):
    g, og = _grids(lom, oracle, knee)
    # (every third point lies over the same plane: a stride of 5 keeps all three planes, and both offsets, in the 100)
    scan = np.ascontiguousarray(knee["scan"][1::5][:n] if n > 1 else knee["scan"][:1])
    assert len(scan) == n
    r = _residuals_at(oracle, og, scan, GUESS)
    assert len(r) == n
    if n > 1:
        assert np.sum((r > 0.15) & (r < 0.3)) * 3 >= n
    for outer in ((0, 1) if n > 1 else (0,)):     # (n = 1: the evaluation at the guess, see the top of the file)
        pose, st, ne, excess, s0 = _trace_vs_oracle(lom, oracle, g, og, scan, lom.Pose3D(*GUESS), outer, ("few", n), n > 1)
        assert ne >= 2
    assert st["queries"] > 0 and s0[28] == n
    _align_vs_oracle(lom, oracle, g, og, scan, GUESS, st, pose)
