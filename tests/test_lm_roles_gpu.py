"""k_lm's 256-thread shapes run a policy wave of their own next to four point waves.  Solves that take many outer
iterations, at the C2 shape (two register points per lane, > 16,384 points) and at the C5 shape (one per lane): the
device agrees with the oracle, and the single, batch and multi-map forms agree bit for bit."""
import numpy as np
import pytest

from tests import scenes
from tests.test_align_batch_gpu import _assert_equal

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4


@pytest.fixture(scope="module")
def world(lom, oracle):
    from lidar_odometry_demo_amd import synth as S

    boxes = S.make_boxes()
    mp, mn = S.make_map_points(300_000, boxes=boxes)
    vlp, _, _, _ = S.make_scan(16, 1800, boxes=boxes)
    g = lom.VoxelGrid(0.5, 20)
    g.addCloud(mp, mn)
    og = oracle.VoxelGrid(0.5, 20)
    og.addCloud(mp, mn)
    rng = np.random.default_rng(11)
    small = np.ascontiguousarray(vlp[np.sort(rng.choice(len(vlp), 12_000, replace=False))])
    return g, og, np.ascontiguousarray(vlp), small


def _far_guesses():
    """off by decimetres and several degrees: solves of six or seven outer iterations and up to 28 evaluations"""
    return [((0.35, -0.3, 0.05), scenes.angle_axis_q(0.06, (0, 0, 1))),
            ((0.0, 0.0, 0.0), scenes.angle_axis_q(0.1, (1, 0, 0))),
            ((0.0, 0.0, 0.2), scenes.angle_axis_q(0.08, (0, 1, 0))),
            ((0.0, 0.0, 0.0), scenes.angle_axis_q(0.25, (0, 0, 1)))]


def _agree_with_oracle(lom, oracle, g, og, scan, t, q):
    m, om = lom.CloudMatcher(), oracle.CloudMatcher(nthreads=8)
    p = m.align(g, scan, lom.Pose3D(t, q))
    o = om.align(og, scan, oracle.Pose3D(t, q))
    dt, dr = scenes.pose_delta(p.translation, p.rotation, o.translation, o.rotation)
    assert dt < POSE_TOL and dr < POSE_TOL, (t, dt, dr)
    for k in ("outer_iterations", "lm_iterations", "queries", "valid_last"):
        assert m.stats[k] == om.stats[k], (t, k, m.stats[k], om.stats[k])
    assert m.stats["evaluations"] == om.stats["points_evaluated"], t
    assert not m.stats["host_fallback"]
    return m.stats


@pytest.mark.parametrize("shape", ["C2", "C5"])
def test_far_guesses_agree_with_oracle(lom, oracle, world, shape):
    g, og, vlp, small = world
    scan = vlp if shape == "C2" else small
    assert (len(scan) > 16_384) == (shape == "C2")
    outers = []
    for t, q in _far_guesses():
        st = _agree_with_oracle(lom, oracle, g, og, scan, t, q)
        outers.append(st["outer_iterations"])
        # several trial steps per solve
        assert st["evaluations"] > 3 * st["outer_iterations"]
    assert min(outers) > 5


@pytest.mark.parametrize("shape", ["C2", "C5"])
def test_single_batch_and_multi_forms_bit_equal(lom, world, shape):
    g, _, vlp, small = world
    scan = vlp if shape == "C2" else small
    guesses = [lom.Pose3D(t, q) for t, q in _far_guesses()] + [lom.Pose3D((0.02, -0.01, 0.0), (1, 0, 0, 0))]
    m = lom.CloudMatcher()
    singles = []
    for gs in guesses:
        p = m.align(g, scan, gs)
        singles.append((p, dict(m.stats)))
    clouds = [scan] * len(guesses)
    batch = m.alignBatch(g, clouds, guesses)
    _assert_equal(batch, m.batch_stats, singles)
    multi = m.alignMulti([g] * len(guesses), clouds, guesses)
    _assert_equal(multi, m.batch_stats, singles)
