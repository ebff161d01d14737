"""Whole aligns that take the branches of the LM policy a healthy align rarely takes, through k_lm itself.

tests/test_lm_policy_gpu.py covers csrc/lm_wave.hpp on given sums; it does not cover what k_lm does with an early LM_DONE
out of the policy's begin, or with a solve whose steps are rejected.  Here tiny maps and scans of 7 to 2,000 points (the
256-thread kernels, policy state in registers) plus one scan of more than 16,384 points (the 512-thread kernels, policy
state in LDS) are aligned against the oracle at the 1e-4 m / 1e-4 rad bars with equal LM numbers
(_assert_lm_numbers of test_eval_parity.py), once as single aligns and once as ONE alignBatch of the same problems, whose
results must be bit-equal to the singles.

* single plane: the rotation about the normal and the in-plane translation are unobservable (minimum-diagonal clamp);
* zero normals: every evaluation is exactly zero, each solve ends in the policy's begin (gradient tolerance at
  iteration 0) and the align in its fifth outer iteration without having moved;
* two planes 1e-4 rad apart: an ill-conditioned translation block;
* a corner of 0.5 m near the origin and guesses 0.3 to 1 rad off, picked with the oracle alone for their rejected steps,
  at 7 and 20 points and at 17,000 (20 points repeated, so that the 512-thread kernels reject steps too): the oracle's
  counts of rejected steps (orc_align_stats) prove that the branch was reached.

An align's prior is its own guess (cloud_matcher.cpp:153), so "zero normals with the guess off the prior" does not exist
at this level: zero rows of A with a live gradient are covered by the probe's cases (zero_normals_off_prior_*) only.
"""
import numpy as np
import pytest

from tests import scenes
from tests.test_align_batch_gpu import _assert_equal
from tests.test_eval_parity import _assert_lm_numbers

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4


def _planes(rng, normals, offsets, per, half):
    pts, nrm = [], []
    for n, off in zip(normals, offsets):
        n = np.asarray(n, np.float64)
        n = n / np.linalg.norm(n)
        e1 = np.cross(n, [0.31, -0.52, 0.8])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(n, e1)
        uv = rng.uniform(-half, half, (per, 2))
        pts.append(off * n + uv[:, :1] * e1 + uv[:, 1:] * e2)
        nrm.append(np.tile(-n, (per, 1)))
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32)


AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
# (seed of the scan subset and the guess, scan points): chosen on the CPU, with the oracle alone, among seeds 0..1499
FAR_SEEDS = ((255, 7), (416, 20), (1011, 20), (386, 20), (695, 7), (1230, 7))
# the same for the 512-thread kernels: 20 points repeated 850 times (17,000 points), among seeds 0..399
FAR_BIG_SEEDS = (130, 197)


def far_problem(seed, n, pool):
    """a guess 0.3 to 1 rad and up to 5 cm off for `n` points of the corner scan"""
    rng = np.random.default_rng(1000 + seed)
    scan = np.ascontiguousarray(pool[np.sort(rng.choice(len(pool), n, replace=False))])
    q = scenes.angle_axis_q(float(rng.uniform(0.3, 1.0)), scenes._unit(rng.standard_normal(3).astype(np.float32)))
    return scan, rng.uniform(-0.05, 0.05, 3).astype(np.float32), q


def corner_world():
    """(map points, map normals, voxel size, scan pool): three faces of a 0.5 m corner, 0.2 m from the origin"""
    mp, mn = _planes(np.random.default_rng(3), AXES, (0.2, 0.2, 0.2), 1500, 0.25)
    pool, _ = _planes(np.random.default_rng(4), AXES, (0.2, 0.2, 0.2), 6000, 0.2)
    return mp, mn, 0.1, pool


def problems():
    """[(tag, map xyz, map normals or None, voxel size, scan, guess t, guess q, wants rejected steps)]"""
    out = []
    rng = np.random.default_rng(21)
    # a single plane z = 0
    mp, mn = _planes(rng, ((0, 0, 1),), (0.0,), 4000, 6.0)
    scan, _ = _planes(rng, ((0, 0, 1),), (0.0,), 17000, 5.0)
    for n in (7, 500, 2000, 17000):
        out.append((f"plane_{n}", mp, mn, 0.5, np.ascontiguousarray(scan[:n]), (0.03, -0.02, 0.05),
                    scenes.angle_axis_q(0.01, scenes._unit(np.array((1, 0.5, 0.2), np.float32))), False))
    # zero normals: addCloudWithoutNormals
    out.append(("zero_normals_63", mp, None, 0.5, np.ascontiguousarray(scan[:63]), (0.05, 0.02, 0.01),
                scenes.angle_axis_q(0.02, (0, 0, 1)), False))
    # two planes whose normals are 1e-4 rad apart, 1 m from each other
    mp2, mn2 = _planes(rng, ((0, 0, 1), (1e-4, 0, 1)), (0.0, 1.0), 2500, 5.0)
    sc2, _ = _planes(rng, ((0, 0, 1), (1e-4, 0, 1)), (0.0, 1.0), 1000, 4.0)
    for n in (1200, 2000):
        sel = np.sort(np.random.default_rng(n).choice(len(sc2), n, replace=False))
        out.append((f"near_parallel_{n}", mp2, mn2, 0.5, np.ascontiguousarray(sc2[sel]), (0.02, 0.01, -0.04),
                    scenes.angle_axis_q(0.008, scenes._unit(np.array((1, -1, 0.3), np.float32))), False))
    # far guesses with rejected steps
    cm, cn, voxel, pool = corner_world()
    for seed, n in FAR_SEEDS:
        sc, t, q = far_problem(seed, n, pool)
        out.append((f"far_{seed}_{n}", cm, cn, voxel, sc, t, q, True))
    for seed in FAR_BIG_SEEDS:
        sc, t, q = far_problem(seed, 20, pool)
        out.append((f"far_big_{seed}", cm, cn, voxel, np.ascontiguousarray(np.tile(sc, (850, 1))), t, q, True))
    return out


@pytest.fixture(scope="module")
def solved(lom, oracle):
    """every problem through the oracle and as a single align on the device, maps shared between problems"""
    maps, res = {}, []
    for tag, mp, mn, voxel, scan, t, q, wants in problems():
        key = (id(mp), mn is None)
        if key not in maps:
            g, og = lom.VoxelGrid(voxel, 20), oracle.VoxelGrid(voxel, 20)
            g.setOption(lom.capi.OPT_COUNT_CANDIDATES, 1)   # the reference algorithm's counts: _assert_lm_numbers compares them
            if mn is None:
                g.addCloudWithoutNormals(mp)
                og.addCloudWithoutNormals(mp)
            else:
                g.addCloud(mp, mn)
                og.addCloud(mp, mn)
            maps[key] = (g, og)
        g, og = maps[key]
        om, m = oracle.CloudMatcher(nthreads=8), lom.CloudMatcher()
        ref = om.align(og, scan, oracle.Pose3D(t, q))
        pose = m.align(g, scan, lom.Pose3D(t, q))
        res.append(dict(tag=tag, g=g, scan=scan, guess=lom.Pose3D(t, q), wants=wants, ref=ref, ost=dict(om.stats),
                        pose=pose, st=dict(m.stats)))
    return res


def test_problems_reach_their_branches(solved):
    """from the oracle's numbers alone"""
    by = {r["tag"]: r for r in solved}
    far = [r for r in solved if r["wants"]]
    assert len(far) >= 4
    for r in far:
        assert r["ost"]["rejected_steps"] > 0, r["tag"]
        assert r["ost"]["outer_iterations"] < 35 and r["ost"]["last_step_norm"] < 1e-4, r["tag"]   # it converges
    assert any(r["ost"]["rejected_steps"] >= 3 for r in far)
    assert sum(len(r["scan"]) > 16384 for r in far) >= 2 and sum(len(r["scan"]) <= 20 for r in far) >= 4
    z = by["zero_normals_63"]["ost"]
    # every solve ends in iteration 0: one recorded iteration and one evaluation per outer iteration
    assert z["outer_iterations"] == 5 and z["lm_iterations"] == 5 and z["points_evaluated"] == 5 and z["final_cost"] == 0.0
    assert z["valid_last"] == 63
    assert any(len(r["scan"]) > 16384 for r in solved) and any(len(r["scan"]) == 7 for r in solved)


def test_single_aligns_agree_with_the_oracle(solved):
    for r in solved:
        dt, dr = scenes.pose_delta(r["pose"].translation, r["pose"].rotation, r["ref"].translation, r["ref"].rotation)
        assert dt < POSE_TOL and dr < POSE_TOL, (r["tag"], dt, dr)
        _assert_lm_numbers(r["st"], r["ost"])
        assert not r["st"]["host_fallback"], r["tag"]


def test_batch_is_bit_equal_to_the_singles(lom, solved):
    """one alignBatch per map with all of the map's problems"""
    groups = {}
    for r in solved:
        groups.setdefault(id(r["g"]), []).append(r)
    m = lom.CloudMatcher()
    for rs in groups.values():
        batch = m.alignBatch(rs[0]["g"], [r["scan"] for r in rs], [r["guess"] for r in rs])
        _assert_equal(batch, m.batch_stats, [(r["pose"], r["st"]) for r in rs])
