"""Batched align (lom_match_align_batch / CloudMatcher.alignBatch): K (scan, guess) problems against one keyframe in
one call.  The reference for every case is the single align (lom_match_align*) on the same handle with the same scan
and guess: the batch must return its pose bytes and its counters bit for bit -- in both search modes (product default,
and with the reference-algorithm counts)."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

from tests import cpp_program
from tests import scenes
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

KEYS = ("outer_iterations", "lm_iterations", "evaluations", "match_launches", "queries", "valid_last", "cand_total",
        "occ_total", "lm_workgroups")
FKEYS = ("final_cost", "last_step_norm")


@pytest.fixture(autouse=True, params=["product", "counted"])
def search_mode(request, monkeypatch):
    """every test twice: handles as a caller gets them, and with LOM_COUNT_CANDIDATES=1 at create"""
    monkeypatch.setenv("LOM_COUNT_CANDIDATES", "1" if request.param == "counted" else "0")
    return request.param


def _bits(p):
    return np.asarray(p.translation, np.float32).tobytes() + np.asarray(p.rotation, np.float32).tobytes()


def _singles(lom, keyframe, clouds, guesses):
    m = lom.CloudMatcher()
    out = []
    for c, g in zip(clouds, guesses):
        p = m.align(keyframe, c, g)
        out.append((p, dict(m.stats)))
    return out


def _assert_equal(batch_poses, batch_stats, singles, fallback=None):
    assert len(batch_poses) == len(singles) == len(batch_stats)
    for i, (bp, bs, (sp, ss)) in enumerate(zip(batch_poses, batch_stats, singles)):
        assert _bits(bp) == _bits(sp), (i, bp, sp)
        for k in KEYS:
            assert bs[k] == ss[k], (i, k, bs[k], ss[k])
        for k in FKEYS:
            assert np.float64(bs[k]).tobytes() == np.float64(ss[k]).tobytes(), (i, k, bs[k], ss[k])
        want_fb = 0 if fallback is None else fallback[i]
        assert bs["host_fallback"] == want_fb, (i, bs["host_fallback"])
        assert bs["match_kernel_ms"] == 0.0 and bs["profiled_launches"] == 0


def _best_of(lom, singles):
    r = (lom.capi.AlignResult * len(singles))()
    for i, (_, st) in enumerate(singles):
        r[i].stats.valid_last = st["valid_last"]
        r[i].stats.final_cost = st["final_cost"]
    return lom.capi.lib().lom_align_batch_best(r, len(singles))


@pytest.fixture(scope="module")
def matching(fixture_cloud):
    """run_matching_test's inputs (test/test.cpp:226-248): keyframe data and the seven guess clouds"""
    import lidar_odometry_demo_amd as lom

    xyz, xyzn = fixture_cloud
    vf = lom.VoxelGrid(0.5, 1)
    vf.addCloudWithoutNormals(xyz)
    sub = vf.getCloudWithoutNormals()
    clouds, truths = [], []
    for t, q in scenes.matching_guess_poses()[:7]:
        guess = lom.Pose3D(t, q)
        truths.append(guess)
        clouds.append(lom.transform_points(guess.inverse(), sub))
    return xyzn, clouds, truths


def _keyframe(lom, xyzn):
    g = lom.VoxelGrid(0.25, 20)
    g.addCloud(xyzn[:, :3], xyzn[:, 3:])
    return g


def _synth_problems(lom, k=12, seed=7):
    """one scan from k seeded guesses: small perturbations, one far one (many outer iterations) and one with no
    correspondence at all (the solve stays at the guess)"""
    rng = np.random.default_rng(seed)
    guesses = []
    for i in range(k - 2):
        t = rng.uniform(-0.08, 0.08, 3)
        q = scenes.angle_axis_q(float(rng.uniform(-0.02, 0.02)), (0, 0, 1))
        guesses.append(lom.Pose3D(t, q))
    guesses.append(lom.Pose3D((0.35, -0.3, 0.05), scenes.angle_axis_q(0.06, (0, 0, 1))))
    guesses.append(lom.Pose3D((500.0, 0.0, 0.0), (1, 0, 0, 0)))
    return guesses


@pytest.fixture(scope="module")
def synth():
    return scenes.small_synth_case()


def _synth_grid(lom, sm):
    g = lom.VoxelGrid(0.5, 20)
    g.addCloud(sm["map_xyz"], sm["map_nrm"])
    return g


# ---- 1. MatchingTest as one call -------------------------------------------------------------------------------------

def test_matching_test_as_one_batch(lom, matching, search_mode):
    xyzn, clouds, truths = matching
    g = _keyframe(lom, xyzn)
    guesses = [lom.Pose3D() for _ in clouds]
    m = lom.CloudMatcher()
    poses = m.alignBatch(g, clouds, guesses)
    singles = _singles(lom, g, clouds, guesses)
    _assert_equal(poses, m.batch_stats, singles)
    assert m.best == _best_of(lom, singles)
    with open(os.path.join(GOLDEN, "c1_matching_test.json")) as f:
        gold = json.load(f)
    for p, st, gc in zip(poses, m.batch_stats, gold["cases"]):
        dt, dr = scenes.pose_delta(p.translation, p.rotation, gc["final_t"], gc["final_q_wxyz"])
        assert dt < 1e-4 and dr < 1e-4, (dt, dr)
        assert st["outer_iterations"] == gc["stats"]["outer_iterations"]
        assert st["valid_last"] == gc["stats"]["valid_last"]


# ---- 2. one scan, K guesses ------------------------------------------------------------------------------------------

def test_one_scan_many_guesses(lom, synth):
    g = _synth_grid(lom, synth)
    guesses = _synth_problems(lom)
    clouds = [synth["scan"]] * len(guesses)
    m = lom.CloudMatcher()
    poses = m.alignBatch(g, clouds, guesses)
    singles = _singles(lom, g, clouds, guesses)
    _assert_equal(poses, m.batch_stats, singles)
    assert max(st["outer_iterations"] for _, st in singles) > 5
    assert singles[-1][1]["valid_last"] == 0 and _bits(poses[-1]) == _bits(guesses[-1])
    assert m.best == _best_of(lom, singles)


def test_shared_cloud_behind_another_on_a_handle_that_has_to_grow(lom, synth):
    """the staging's other branches: a cloud several problems share that is not the call's first (an empty problem and a
    second shared cloud between its uses), on a handle whose pinned blocks -- staged descriptors, report slots -- were
    sized by a first call of two problems and grow for this one of twenty"""
    g = _synth_grid(lom, synth)
    scan = np.ascontiguousarray(synth["scan"], np.float32)
    other = np.ascontiguousarray(scan[:300])
    m = lom.CloudMatcher()
    two = [lom.Pose3D(), lom.Pose3D()]
    first = m.alignBatch(g, [other, scan], two)
    guesses = _synth_problems(lom, k=20, seed=3)
    clouds = [other, scan, scan, scan[:0], other] + [scan] * 15
    poses = m.alignBatch(g, clouds, guesses)
    _assert_equal(poses, m.batch_stats, _singles(lom, g, clouds, guesses))
    again = m.alignBatch(g, [other, scan], two)
    assert [_bits(p) for p in again] == [_bits(p) for p in first]


# ---- 3. mixed sizes: several groups in one call ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    from lidar_odometry_demo_amd import synth as S

    boxes = S.make_boxes()
    mp, mn = S.make_map_points(300_000, boxes=boxes)
    vlp, _, _, _ = S.make_scan(16, 1800, boxes=boxes)        # C2-sized: 256 threads, two points per lane
    big, _, _, _ = S.make_scan(32, 1800, boxes=boxes)        # >= 40k points: the 512-thread shape
    return mp, mn, vlp, big


def test_mixed_sizes_one_call(lom, mixed):
    mp, mn, vlp, big = mixed
    g = lom.VoxelGrid(0.5, 20)
    g.addCloud(mp, mn)
    clouds = [vlp[:0], vlp[:1], vlp[:7], vlp[:500], vlp[:2048], vlp, big, vlp[:20000], big[:45000]]
    assert len(big) >= 40000
    guesses = [lom.Pose3D((0.02 * i, -0.01 * i, 0.0), scenes.angle_axis_q(0.003 * i, (0, 0, 1))) for i in range(len(clouds))]
    m = lom.CloudMatcher()
    poses = m.alignBatch(g, clouds, guesses)
    singles = _singles(lom, g, clouds, guesses)
    _assert_equal(poses, m.batch_stats, singles)
    assert len({st["lm_workgroups"] for st in m.batch_stats}) >= 4  # several groups


# ---- 4. several rounds -----------------------------------------------------------------------------------------------

def test_several_rounds_same_result(lom, synth):
    g = _synth_grid(lom, synth)
    guesses = _synth_problems(lom, k=8, seed=11)
    clouds = [synth["scan"]] * 8
    m = lom.CloudMatcher()
    one = m.alignBatch(g, clouds, guesses)
    st_one = m.batch_stats
    g.setOption(lom.capi.OPT_TEST_BATCH_ROUND_MAX, 3)
    three = m.alignBatch(g, clouds, guesses)
    assert [s["round"] for s in m.batch_stats] == [0, 0, 0, 1, 1, 1, 2, 2]
    _assert_equal(three, m.batch_stats, list(zip(one, st_one)))
    g.setOption(lom.capi.OPT_TEST_BATCH_ROUND_MAX, 0)
    _assert_equal(one, st_one, _singles(lom, g, clouds, guesses))


# ---- 5. give-up --------------------------------------------------------------------------------------------------------

def test_give_up_redoes_that_problem_alone(lom, synth):
    g = _synth_grid(lom, synth)
    guesses = _synth_problems(lom, k=5, seed=3)[:4]
    clouds = [synth["scan"]] * len(guesses)
    singles = _singles(lom, g, clouds, guesses)
    g.setOption(lom.capi.OPT_TEST_GIVE_UP_AT_OUTER, 2)
    m = lom.CloudMatcher()
    poses = m.alignBatch(g, clouds, guesses)
    _assert_equal(poses, m.batch_stats, singles, fallback=[1, 0, 0, 0])
    # one shot: the next batch runs on the device throughout
    poses = m.alignBatch(g, clouds, guesses)
    _assert_equal(poses, m.batch_stats, singles)


# ---- 6. host-driven loop -----------------------------------------------------------------------------------------------

def test_host_lm_batch_equals_host_singles(lom, synth):
    g = _synth_grid(lom, synth)
    g.setOption(lom.capi.OPT_HOST_LM, 1)
    guesses = _synth_problems(lom, k=4, seed=5)
    clouds = [synth["scan"], synth["scan"][:300], synth["scan"], synth["scan"][:0]]
    m = lom.CloudMatcher()
    poses = m.alignBatch(g, clouds, guesses)
    _assert_equal(poses, m.batch_stats, _singles(lom, g, clouds, guesses))


# ---- 7. isolation --------------------------------------------------------------------------------------------------------

def test_single_batch_single_identical(lom, synth):
    g = _synth_grid(lom, synth)
    guesses = _synth_problems(lom, k=6, seed=9)
    m = lom.CloudMatcher()
    before = m.align(g, synth["scan"], guesses[0])
    st_before = dict(m.stats)
    m.alignBatch(g, [synth["scan"][:1000]] * 6, guesses)
    after = m.align(g, synth["scan"], guesses[0])
    assert _bits(before) == _bits(after)
    for k in KEYS + FKEYS:
        assert st_before[k] == m.stats[k]


def test_batch_leaves_cleanup_and_idle_hook_armed(lom, synth):
    guesses = _synth_problems(lom, k=4, seed=13)
    L = lom.capi.lib()
    HOOK = C.CFUNCTYPE(None, C.c_void_p)
    calls = []
    hook = HOOK(lambda user: calls.append(1))
    L.lom_map_set_align_idle_hook.argtypes = [C.c_void_p, HOOK, C.c_void_p]
    exports = []
    for with_batch in (False, True):
        g = _synth_grid(lom, synth)
        m = lom.CloudMatcher()
        g.radiusCleanupAfterAlign(12.0)
        L.lom_map_set_align_idle_hook(g.handle, hook, None)
        if with_batch:
            n_calls = len(calls)
            m.alignBatch(g, [synth["scan"]] * 4, guesses)
            assert len(calls) == n_calls                         # the batch does not run the hook
        p = m.align(g, synth["scan"], guesses[0])
        g.radiusCleanup(p.translation, 12.0)
        xyz, nrm = g.getCloud()
        exports.append((xyz.tobytes(), nrm.tobytes(), g.size()))
    assert exports[0] == exports[1]
    assert len(calls) == 2                                       # each single align ran it once


# ---- 8. two threads on partitioned contexts ----------------------------------------------------------------------------

def test_two_partitioned_contexts_in_threads(lom, synth):
    g = _synth_grid(lom, synth)
    jobs = [_synth_problems(lom, k=6, seed=21), _synth_problems(lom, k=6, seed=22)]
    alone = []
    for guesses in jobs:
        m = lom.CloudMatcher()
        alone.append((m.alignBatch(g, [synth["scan"]] * 6, guesses), m.batch_stats))
    ctxs = [lom.ScanContext(g, partition=(i, 2)) for i in range(2)]
    got = [None, None]
    errors = []

    def work(i):
        try:
            m = lom.CloudMatcher()
            for _ in range(3):
                got[i] = (m.alignBatch(ctxs[i], [synth["scan"]] * 6, jobs[i]), m.batch_stats)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for i in range(2):
        poses, stats = got[i]
        # (a context on a partition may give a problem up and redo it: same bits, host_fallback set)
        fb = [s["host_fallback"] for s in stats]
        _assert_equal(poses, stats, list(zip(*alone[i])), fallback=fb)
    for c in ctxs:
        c.close()


# ---- 9. device and host variants; repeatability --------------------------------------------------------------------------

def test_device_variant_equals_host_and_repeats(lom, synth):
    import torch

    g = _synth_grid(lom, synth)
    guesses = _synth_problems(lom, k=6, seed=31)
    clouds = [synth["scan"], synth["scan"][:900], synth["scan"][:0], synth["scan"], synth["scan"][::2], synth["scan"][:1]]
    m = lom.CloudMatcher()
    host = m.alignBatch(g, clouds, guesses)
    host_stats = m.batch_stats
    tensors = [torch.from_numpy(np.ascontiguousarray(c, np.float32)).to("cuda:0") for c in clouds]
    torch.cuda.synchronize()
    items = [(t.data_ptr() if len(c) else None, len(c), gs) for t, c, gs in zip(tensors, clouds, guesses)]
    ref = list(zip(host, host_stats))
    for _ in range(50):
        dev = m.alignBatchDevice(g, items)
        _assert_equal(dev, m.batch_stats, ref)
    _assert_equal(host, host_stats, _singles(lom, g, clouds, guesses))


# ---- 10. mirrors ---------------------------------------------------------------------------------------------------------

def test_python_mirror_on_scan_context(lom, synth):
    g = _synth_grid(lom, synth)
    guesses = _synth_problems(lom, k=5, seed=41)
    clouds = [synth["scan"]] * 5
    cx = lom.ScanContext(g)
    m = lom.CloudMatcher()
    poses = m.alignBatch(cx, clouds, guesses)
    _assert_equal(poses, m.batch_stats, _singles(lom, g, clouds, guesses))
    assert m.best == _best_of(lom, _singles(lom, cx, clouds, guesses))
    assert m.alignBatch(cx, [], []) == [] and m.best == -1
    cx.close()


def test_cpp_mirror_align_batch(tmp_path, lom):
    exe = cpp_program.build_with_library(tmp_path, "test_batch.cpp")
    cpp_program.run(exe, timeout=300)
