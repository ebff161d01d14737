"""Replay fold on the device (k_lm's tail, LOM_OPT_REPLAY_FOLD): with the fold on and off the single align returns the same
pose bytes and the same statistics -- the statistics describe the reference algorithm's align, folded iterations
included -- while lom_debug_replayed_iterations tells how many (k_match, k_lm) pairs did no work.

Shapes: the smallest scan of every form of k_lm -- 256 threads with one point per lane, with two points per lane, 512
threads on up to 64 and on up to 128 workgroups.  Guesses: the identity (the host test shows the fifth iteration of
`small_synth_case` repeating the fourth) and one offset."""
import pytest

from tests import scenes

pytestmark = pytest.mark.gpu

# fields that are times, not counts
TIMES = ("host_launch_ms", "host_wait_ms", "match_kernel_ms", "lm_kernel_ms")

SHAPES = {
    "one_point_per_lane": lambda: scenes.small_synth_case(),              # 2,048 points: k_lm<256>
    "two_points_per_lane": lambda: scenes.synth_case(16, 1300, 100_000),   # 16,385..32,768: k_lm<256, 64, 2>
    "512_threads": lambda: scenes.synth_case(64, 640, 100_000),            # 32,769..65,536: k_lm<512>
    "512_threads_128_workgroups": lambda: scenes.synth_case(128, 640, 100_000),  # above: k_lm<512, 128>
}
GUESSES = {
    "identity": ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)),
    "offset": ((0.1, -0.05, 0.02), tuple(scenes.angle_axis_q(0.01, (0, 0, 1)))),
}


def _counts(stats):
    return {k: v for k, v in stats.items() if k not in TIMES}


@pytest.fixture(scope="module")
def cases():
    return {}


def _case(cases, shape):
    if shape not in cases:
        cases[shape] = SHAPES[shape]()
    return cases[shape]


def _grid(lom, case, count=False):
    g = lom.VoxelGrid(0.5, 20)
    g.addCloud(case["map_xyz"], case["map_nrm"])
    if count:
        g.setOption(lom.capi.OPT_COUNT_CANDIDATES, 1)
    return g


def _align(lom, g, case, guess, fold):
    g.setOption(lom.capi.OPT_REPLAY_FOLD, 1 if fold else 0)
    m = lom.CloudMatcher()
    pose = m.align(g, case["scan"], lom.Pose3D(*guess))
    assert m.stats["host_fallback"] == 0
    return pose.translation.tobytes() + pose.rotation.tobytes(), m.stats, g.replayedIterations()


@pytest.mark.parametrize("count", [False, True], ids=["default", "count_candidates"])
@pytest.mark.parametrize("guess", list(GUESSES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fold_on_and_off_agree(lom, cases, shape, guess, count):
    case = _case(cases, shape)
    lanes = {"one_point_per_lane": (1, 16384), "two_points_per_lane": (16385, 32768), "512_threads": (32769, 65536),
             "512_threads_128_workgroups": (65537, 1 << 31)}[shape]
    assert lanes[0] <= len(case["scan"]) <= lanes[1], len(case["scan"])
    g = _grid(lom, case, count)
    pose_off, st_off, rep_off = _align(lom, g, case, GUESSES[guess], False)
    pose_on, st_on, rep_on = _align(lom, g, case, GUESSES[guess], True)
    print(shape, guess, "outer", st_off["outer_iterations"], "evaluations", st_off["evaluations"], "replayed", rep_on)
    assert rep_off == 0
    assert pose_on == pose_off
    assert _counts(st_on) == _counts(st_off)
    assert st_on["match_launches"] == st_on["outer_iterations"]
    assert st_on["queries"] == st_on["outer_iterations"] * len(case["scan"])
    assert 0 <= rep_on < st_on["outer_iterations"]
    if count:
        assert st_on["cand_total"] > 0 and st_on["occ_total"] > 0 and st_on["algorithmic_bytes"] > 0
        for k in ("cand_total", "occ_total", "algorithmic_bytes"):
            assert st_on[k] == st_off[k], k
    if shape == "one_point_per_lane" and guess == "identity":
        assert rep_on >= 1      # tests/test_replay_fold_host.py: iteration 5 searches at iteration 4's pose


@pytest.mark.parametrize("shape", list(SHAPES))
def test_align_after_a_folded_align_is_undisturbed(lom, cases, shape):
    """The kernels enqueued for the folded iterations return at once, between the two aligns, on one handle."""
    case = _case(cases, shape)
    fresh = _grid(lom, case)
    want_pose, want_st, _ = _align(lom, fresh, case, GUESSES["offset"], True)
    g = _grid(lom, case)
    _, st1, rep1 = _align(lom, g, case, GUESSES["identity"], True)
    pose2, st2, _ = _align(lom, g, case, GUESSES["offset"], True)
    print(shape, "first align replayed", rep1)
    assert pose2 == want_pose
    assert _counts(st2) == _counts(want_st)
    if shape == "one_point_per_lane":
        assert rep1 >= 1


@pytest.mark.parametrize("shape", list(SHAPES))
def test_profiled_launches_count_the_pairs_that_ran(lom, cases, shape):
    """An align that carries the profiling events runs every pair it brackets (tests/test_gpu_parity.py,
    test_sampled_profiling_events: profiled_launches == match_launches), so nothing is folded in it; the aligns between
    the sampled ones fold."""
    case = _case(cases, shape)
    g = _grid(lom, case)
    g.setProfiling(1)
    for guess in GUESSES.values():
        for fold in (False, True):
            _, st, rep = _align(lom, g, case, guess, fold)
            assert st["profiled_launches"] == st["outer_iterations"] - rep
            assert st["lm_profiled_launches"] == st["outer_iterations"] - rep
            assert st["profiled_launches"] == st["match_launches"]
            assert st["match_kernel_ms"] > 0 and st["lm_kernel_ms"] > 0
    if shape == "one_point_per_lane":
        g.setProfiling(2)       # the first align carries the events, the second does not
        _, st_a, rep_a = _align(lom, g, case, GUESSES["identity"], True)
        _, st_b, rep_b = _align(lom, g, case, GUESSES["identity"], True)
        assert st_a["profiled_launches"] == st_a["outer_iterations"] and rep_a == 0
        assert st_b["profiled_launches"] == 0 and rep_b >= 1
        assert _counts({**st_a, "profiled_launches": 0, "lm_profiled_launches": 0}) == _counts(st_b)


def test_scan_context_inherits_the_option(lom, cases):
    case = _case(cases, "one_point_per_lane")
    g = _grid(lom, case)
    g.setOption(lom.capi.OPT_REPLAY_FOLD, 0)
    ctx = lom.ScanContext(g)
    m = lom.CloudMatcher()
    off = m.align(ctx, case["scan"], lom.Pose3D())
    assert lom.capi.replayed_iterations(ctx.handle) == 0
    ctx.setOption(lom.capi.OPT_REPLAY_FOLD, 1)
    on = m.align(ctx, case["scan"], lom.Pose3D())
    assert lom.capi.replayed_iterations(ctx.handle) >= 1
    assert on.translation.tobytes() == off.translation.tobytes() and on.rotation.tobytes() == off.rotation.tobytes()


def test_an_exchange_with_one_rank_folds_like_no_exchange(lom, cases):
    """A communicator with a single rank exchanges nothing (px.nranks == 1): the align folds, and costs, the same with
    it attached as without (bench.py's LOM_BENCH_FORCE_DIST rehearsal must give the --gpus 1 figure).  Device-to-device
    exchange: the chained align; host exchange: the host-driven loop, where the driver's own switch turns the fold off."""
    import ctypes as C

    case = _case(cases, "one_point_per_lane")
    L = lom.capi.lib()
    want_pose, want_st, want_rep = _align(lom, _grid(lom, case), case, GUESSES["identity"], True)
    assert want_rep >= 1
    ident = C.create_string_buffer(lom.capi.COMM_ID_BYTES)
    lom.capi.check(L.lom_comm_host_id(ident))
    hc = C.c_void_p()
    lom.capi.check(L.lom_host_comm_create(0, 1, ident.raw, C.byref(hc)))
    g = _grid(lom, case)
    try:
        lom.capi.check(L.lom_comm_attach_p2p(g.handle, hc), g.handle)
        pose_off, st_off, rep_off = _align(lom, g, case, GUESSES["identity"], False)
        pose_on, st_on, rep_on = _align(lom, g, case, GUESSES["identity"], True)
        assert rep_off == 0 and rep_on == want_rep
        assert pose_on == pose_off == want_pose
        assert _counts(st_on) == _counts(st_off) == _counts(want_st)
        # the host-driven loop over the host exchange, one rank
        lom.capi.check(L.lom_comm_attach_host(g.handle, hc), g.handle)
        m = lom.CloudMatcher()
        got = []
        for on in (0, 1):
            prev = lom.capi.set_host_replay_fold(on)
            try:
                p = m.align(g, case["scan"], lom.Pose3D(*GUESSES["identity"]))
            finally:
                lom.capi.set_host_replay_fold(prev)
            got.append((p.translation.tobytes() + p.rotation.tobytes(), _counts(m.stats)))
        assert got[0] == got[1]
        assert got[0][1]["outer_iterations"] == want_st["outer_iterations"]
    finally:
        L.lom_comm_finalize(g.handle)
        L.lom_host_comm_destroy(hc)
