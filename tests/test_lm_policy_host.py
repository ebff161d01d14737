"""The LM policy of csrc/lm_core.hpp (form 0 of lom_debug_lm_policy, host code) against the independent reference
tests/lm_ref.py, branch by branch, on the small problems of tests/lm_cases.py; plus the conditions that keep that
comparison (and its GPU twin tests/test_lm_policy_gpu.py, same cases, the wave forms of csrc/lm_wave.hpp) honest:

* the generator's restatement of the residual / Jacobian / loss is pinned against the oracle's evaluator;
* a case is admitted only if every threshold comparison the reference made is at least 1e-6 (relative) from flipping --
  orders above any rounding of the bound below -- so a different decision is a bug; at most 10 % may be dropped;
* every branch named below is taken by at least two admitted cases, judged from the reference's tags alone.

Not reachable with max_num_iterations = 4, and so without a case: kLmMaxRadius and kLmMaxDiag (the radius starts at 1e4
and at most triples per step; scaled diagonals are below 1), and invalid_run >= 5 (the iteration budget ends the loop
first).

Per case: every action, `recorded` and `evaluations` equal the reference's; last_step_norm within 1e-13, cost within
1e-12 relative; every proposed point within the bound lm_ref.point_bound derives from the reference's own 50-digit solve.
"""
import numpy as np
import pytest

from tests import lm_cases, lm_ref

# branch -> the reference's tag that proves it (an evaluation's events), at least two admitted cases each
BRANCHES = {
    "accepted step": "accept",
    "rejected step, the next solve reuses the diagonal": "reject",
    "second rejection in a row": "reject_again",
    "reused diagonal": "reuse_diag",
    "invalid step": "invalid",
    "valid step after invalid ones": "valid_after_invalid",
    "exit by the iteration budget": "budget",
    "gradient tolerance at iteration 0": "gtol0",
    "gradient tolerance after an accepted step": "gtol",
    "parameter tolerance": "ptol",
    "function tolerance": "ftol",
    "minimum diagonal clamp": "clamp",
    "zero row of A": "zero_row",
    "ill-conditioned (cond2 > 1e8)": "illcond",
    "half-angle below 0.05": "ha_lo",
    "half-angle 0.05 to 0.5": "ha_mid",
    "half-angle 0.45 to 0.5 at cond2 < 10 (the short series of lmw2_sinc_cos would miss the bound)": "ha_mid_top",
    "half-angle 0.5 or more": "ha_hi",
    "delta with a zero rotation part": "n2zero",
}


def _events(case):
    return {t for e in case["trace"] for t in e["events"]}


def test_generator_matches_the_oracle_evaluator(oracle):
    """eval_sums against orc_shard_eval_fixed on one case: a small map of three planes, the correspondences of a search,
    an evaluation at a non-unit f64 quaternion away from the search pose, residuals on both sides of the Huber knee."""
    rng = np.random.default_rng(7)
    O, N = lm_cases.planes(rng, lm_cases.BOX, 400, half=3.0)
    O, N = O.astype(np.float32), N.astype(np.float32)
    og = oracle.VoxelGrid(0.5, 20)
    og.addCloud(O, N)
    scan = (O[::9] + rng.uniform(-0.04, 0.04, (len(O[::9]), 3)) + np.float32(0.1) * N[::9]).astype(np.float32)
    pose_t, pose_q = np.array([0.02, -0.01, 0.03], np.float32), np.array([1, 0, 0, 0], np.float32)
    corr = og.findMatchingPairs(scan, oracle.Pose3D(pose_t, pose_q), 0.3)
    ok = corr["index"] >= 0
    assert ok.sum() > 50
    sh = oracle.Shard(og, scan)
    sh.match_eval(pose_t, pose_q, pose_q.astype(np.float64), pose_t.astype(np.float64))
    x = np.array([1.00004, 0.0021, -0.0013, 0.0047, 0.08, -0.06, 0.05])
    ref = sh.eval_fixed(x[:4], x[4:])
    got = lm_cases.eval_sums(scan[ok].astype(np.float64), corr["origin"][ok].astype(np.float64),
                             corr["normal"][ok].astype(np.float64), x)
    assert ref[28] == ok.sum() == got[28]
    r = np.abs(np.sum((lm_cases.rotate(x[:4], scan[ok].astype(np.float64)) + x[4:] - corr["origin"][ok]) * corr["normal"][ok], axis=1))
    assert (r > 0.15).any() and (r < 0.15).any()
    # same f64 terms, added in another order: 1e-12 of the block's scale (the bar of test_eval_parity.py)
    diag = [ref[a * 6 - (a * (a - 1)) // 2] for a in range(6)]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            assert abs(got[k] - ref[k]) <= 1e-12 * np.sqrt(diag[a] * diag[b]) + 64 * lm_ref.EPS * max(diag), (a, b)
            k += 1
    for a in range(6):
        assert abs(got[21 + a] - ref[21 + a]) <= 1e-12 * (np.sqrt(diag[a] * 2 * ref[27]) + abs(ref[21 + a])), a
    assert abs(got[27] - ref[27]) <= 1e-12 * ref[27]


def test_admission_and_branch_coverage():
    admitted, dropped = lm_cases.all_cases()
    total = len(admitted) + len(dropped)
    assert total >= 30
    assert len(dropped) <= 0.10 * total, [c["name"] for c in dropped]
    for c in admitted:
        assert 1 <= len(c["trace"]) <= 5
        exact = c["recipe"] in ("nonfinite", "gtol0")      # built on exact values: admitted as they are
        assert exact or lm_ref.min_margin(c["trace"]) >= lm_cases.MARGIN
    for branch, tag in BRANCHES.items():
        n = sum(tag in _events(c) for c in admitted)
        assert n >= 2, (branch, n)
    # a rejection followed by an accepted step, and two rejections in a row, as sequences
    firsts = ["".join({"accept": "A", "reject": "R", "reject_again": "R"}.get(e["events"][0], "-") for e in c["trace"])
              for c in admitted]
    assert sum("RA" in f for f in firsts) >= 2 and sum("RR" in f for f in firsts) >= 2
    assert any(e.get("cond", 0.0) > 1e8 for c in admitted for e in c["trace"])
    # non-finite A or g: four invalid steps and the exit by the iteration budget, without a second evaluation.  A NaN cost
    # does not enter the linear system: its four steps are valid, each candidate is rejected (rel_dec is NaN), same exit.
    nonfinite = [c for c in admitted if c["recipe"] == "nonfinite"]
    assert len(nonfinite) == 5
    for c in nonfinite:
        ev = [t for e in c["trace"] for t in e["events"]]
        if c["name"].endswith("cost_nan"):
            assert ev.count("reject") + ev.count("reject_again") == 4 and ev[-1] == "budget"
        else:
            assert ev.count("invalid") == 4 and ev[-1] == "budget" and len(c["trace"]) == 1
        assert c["trace"][-1]["recorded"] == 5


def test_reference_traces_are_stable():
    """the reference is deterministic: a second run visits the same points bit for bit (the GPU test shares these)"""
    admitted, _ = lm_cases.all_cases()
    c = admitted[3]
    again = lm_ref.solve(c["x0"], c["prior_b"], lm_cases.sums_fn(c))
    assert [e["tag"] for e in again] == [e["tag"] for e in c["trace"]]
    assert all(np.array_equal(a["point"], b["point"]) for a, b in zip(again, c["trace"]))


def test_lm_core_against_the_reference(lom):
    admitted, _ = lm_cases.all_cases()
    got = lom.debug_lm_policy(0, [lm_cases.as_solve(c) for c in admitted])
    worst = 0.0
    for c, g in zip(admitted, got):
        worst = max(worst, lm_cases.check_solve(c, g, "form 0"))
    print(f"form 0: worst error / bound = {worst:.3g}")
    assert worst > 0.0


def test_entry_rejects_bad_arguments(lom):
    admitted, _ = lm_cases.all_cases()
    x0, pb, sums = lm_cases.as_solve(admitted[0])
    with pytest.raises(lom.LomError):
        lom.debug_lm_policy(4, [(x0, pb, sums)])
    with pytest.raises(lom.LomError):
        lom.debug_lm_policy(0, [(x0, pb, sums[:0])])
