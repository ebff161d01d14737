"""Replay fold, host side (no GPU): the fold rule of csrc/lm_core.hpp against a brute-force restatement of the
reference's outer loop, and the product's host driver (lom_align_with_hooks) over the oracle's evaluators with the fold on
and off -- same pose bytes, same statistics, fewer correspondence searches.

An outer iteration is a pure function of the f32 pose it searches at; one that writes back that very pose is followed, in
the reference, by exact repeats of itself until the stop rule of cloud_matcher.cpp:169-172 (last_step_norm < 1e-4 and
i > 3) or the cap of :117 (35) ends the loop.  The driver accounts for those repeats instead of running them."""
import ctypes as C

import numpy as np
import pytest

from tests import scenes


def _brute_force_further(outer, lsn):
    """The reference's loop, run: iterations 0 .. outer-1 are done, each later one repeats iteration outer-1 (same
    last_step_norm).  Counts the iterations executed beyond `outer`."""
    executed = 0
    for i in range(35):                 # cloud_matcher.cpp:117
        executed = i + 1
        if i + 1 < outer:
            continue                    # an iteration that has already run (and did not stop the loop)
        if lsn < 1e-4 and i > 3:        # :169-172
            break
    return executed - outer


def test_fold_rule_matches_the_loop(lom):
    fold_count = lom.capi.lib().lom_debug_replay_fold_count    # replay_fold_count of csrc/lm_core.hpp
    for lsn in (0.0, 9.9e-5, 1e-4, 1.0):
        for outer in range(1, 36):
            # (an `outer` the stop rule would already have ended the loop at has nothing further)
            want = _brute_force_further(outer, lsn)
            assert fold_count(outer, lsn) == want, (outer, lsn)
            assert outer + want == (35 if lsn >= 1e-4 else max(outer, 5)), (outer, lsn)


class _CountingHooks:
    """lom_align_hooks over an oracle Shard; match_eval goes through Python so that its calls (and the f32 poses handed to
    them) are recorded."""

    def __init__(self, lom, oracle, shard):
        OL = oracle.lib()
        self.poses = []

        def match_eval(user, pt, pq, q, t, out):
            self.poses.append(np.array([pq[0], pq[1], pq[2], pq[3], pt[0], pt[1], pt[2]], np.float32).tobytes())
            return OL.orc_shard_match_eval(shard.handle, pt, pq, q, t, out)

        self._me = lom.capi.MATCH_EVAL_FN(match_eval)
        self._ef = lom.capi.EVAL_FIXED_FN(C.cast(OL.orc_shard_eval_fixed, C.c_void_p).value)
        self._shard = shard
        self.hooks = lom.capi.AlignHooks(shard.handle, self._me, self._ef, lom.capi.ALLREDUCE_FN())


def _align(lom, ch, guess_t, guess_q, fold):
    ch.poses = []
    ot, oq = (C.c_float * 3)(), (C.c_float * 4)()
    st = lom.capi.AlignStats()
    was = lom.capi.set_host_replay_fold(fold)
    try:
        rc = lom.capi.lib().lom_align_with_hooks(C.byref(ch.hooks), lom.capi.f3(guess_t), lom.capi.f4(guess_q), ot, oq,
                                                 C.byref(st))
    finally:
        lom.capi.set_host_replay_fold(was)
    assert rc == 0, rc
    return bytes(ot) + bytes(oq), st.asdict(), list(ch.poses)


def _repeats(poses):
    """1-based iterations whose search pose equals the previous iteration's, bit for bit."""
    return [i + 1 for i in range(1, len(poses)) if poses[i] == poses[i - 1]]


def _check_case(lom, oracle, case, guess_t, guess_q, want_outer, want_repeats):
    g = oracle.VoxelGrid(0.5, 20)
    g.addCloud(case["map_xyz"], case["map_nrm"])
    ch = _CountingHooks(lom, oracle, oracle.Shard(g, case["scan"]))
    pose_off, st_off, poses_off = _align(lom, ch, guess_t, guess_q, False)
    pose_on, st_on, poses_on = _align(lom, ch, guess_t, guess_q, True)
    print("outer", st_off["outer_iterations"], "evaluations", st_off["evaluations"], "repeated iterations",
          _repeats(poses_off), "searches with the fold", len(poses_on))
    # the unfolded run shows the pattern the fold relies on ...
    assert st_off["outer_iterations"] == want_outer == len(poses_off)
    assert _repeats(poses_off) == want_repeats
    # ... and the fold changes nothing but the number of searches
    assert pose_on == pose_off
    assert st_on == st_off
    folded = len(want_repeats)
    assert len(poses_on) == st_on["outer_iterations"] - folded
    assert poses_on == poses_off[:len(poses_on)]
    return st_on, len(poses_on)


OFFSET_C2 = ((0.1, -0.05, 0.02), 0.01)


@pytest.fixture(scope="module")
def c2_case():
    """The bench workload (C2): a VLP16 scan, 16 beams x 1800 azimuth steps, against the 500k-point map."""
    return scenes.synth_case(16, 1800, 500_000)


def test_host_fold_c2_identity_guess(lom, oracle, c2_case):
    _check_case(lom, oracle, c2_case, (0, 0, 0), (1, 0, 0, 0), 5, [5])


def test_host_fold_c2_offset_guess(lom, oracle, c2_case):
    t, a = OFFSET_C2
    _check_case(lom, oracle, c2_case, t, scenes.angle_axis_q(a, (0, 0, 1)), 5, [4, 5])


def test_host_fold_small_synth_identity_guess(lom, oracle):
    st, searches = _check_case(lom, oracle, scenes.small_synth_case(), (0, 0, 0), (1, 0, 0, 0), 5, [5])
    assert searches == 4 and st["outer_iterations"] == 5


def test_host_fold_small_synth_offset_guess_runs_six(lom, oracle):
    st, searches = _check_case(lom, oracle, scenes.small_synth_case(), (0.2, -0.2, 0.0),
                               scenes.angle_axis_q(0.01, (0, 0, 1)), 6, [])
    assert searches == 6


def test_host_fold_is_off_with_an_allreduce_hook(lom, oracle):
    """Ranks that exchange sums are out of scope: with hooks->allreduce set every iteration runs."""
    case = scenes.small_synth_case()
    g = oracle.VoxelGrid(0.5, 20)
    g.addCloud(case["map_xyz"], case["map_nrm"])
    ch = _CountingHooks(lom, oracle, oracle.Shard(g, case["scan"]))
    ar = lom.capi.ALLREDUCE_FN(lambda user, sums, n: 0)
    ch.hooks.allreduce = ar
    _, st, poses = _align(lom, ch, (0, 0, 0), (1, 0, 0, 0), True)
    assert len(poses) == st["outer_iterations"] == 5
