"""The seeded walks of tests/map_walks.py on the device beside the oracle: about 30 public calls per seed -- inserts
(also through the no-wait entry), radius cleanups, the cleanup scan behind an align with and without a reader in
between, the cap up and down, exports, searches, a clear -- and the device map is the oracle's all the way.

Bars as tests/test_gpu_parity.py: sizes, exports and searches bit-exact; the closing align within POSE_TOL_M /
POSE_TOL_RAD with equal outer iterations."""
import pytest

from tests import map_walks as W
from tests import scenes
from tests.test_gpu_parity import POSE_TOL_M, POSE_TOL_RAD, _assert_same_map, _assert_same_pairs

pytestmark = pytest.mark.gpu

# every seed in both search modes (as tests/test_gpu_parity.py's search_mode); two seeds also with every cleanup closing
# its holes at once
VARIANTS = [(seed, mode) for seed in W.SEEDS for mode in ("product", "counted")] + [(seed, "dense") for seed in W.DENSE_SEEDS]


@pytest.mark.parametrize("seed,variant", VARIANTS)
def test_walk_equals_the_oracle(lom, oracle, monkeypatch, seed, variant):
    monkeypatch.setenv("LOM_COUNT_CANDIDATES", "1" if variant == "counted" else "0")
    if variant == "dense":
        monkeypatch.setenv("LOM_DENSE_CLEANUP", "1")
    c, w = W.case(), W.walk(seed)
    taken, holes = lom.capi.COUNTER_CLEANUPS_BEHIND_ALIGN, lom.capi.COUNTER_EMPTY_SLABS
    seen = dict(holes=[0])
    last = len(w["steps"]) - 1

    def same_map_and_pairs(g, og):
        _assert_same_map(g, og)
        _assert_same_pairs(g.findMatchingPairs(c["queries"], lom.Pose3D(), 0.3), og.findMatchingPairs(c["queries"], oracle.Pose3D(), 0.3))

    def after(i, step, g, og, info):
        if step[0] in W.MUTATING:
            assert g.size() == og.size() and g.pointCount() == og.pointCount(), (i, step[0])
            seen["holes"].append(g.debugCounter(holes))
        if i % 5 == 4 or i == last:
            same_map_and_pairs(g, og)

    g, og = W.play(w, oracle, lom, after)
    assert g.debugCounter(taken) >= 1, "no cleanup took the scan behind its align"
    h = seen["holes"]
    if variant == "dense":
        assert max(h) == 0
    else:  # empty slabs piled up and were closed later (tests/test_map_walks_host.py: small_then_big)
        assert max(h) > 0 and any(b < a for a, b in zip(h, h[1:])), h
    assert lom.capi.lib().lom_map_status(g.handle) == 0
    m, om = lom.CloudMatcher(), oracle.CloudMatcher()
    p, op = m.align(g, c["scan"], lom.Pose3D(*W.GUESS)), om.align(og, c["scan"], oracle.Pose3D(*W.GUESS))
    dt, dr = scenes.pose_delta(p.translation, p.rotation, op.translation, op.rotation)
    assert dt < POSE_TOL_M and dr < POSE_TOL_RAD and m.stats["outer_iterations"] == om.stats["outer_iterations"]
