"""The wave forms of the LM policy (csrc/lm_wave.hpp) against the independent reference tests/lm_ref.py, branch by branch.

lom_debug_lm_policy replays every admitted case of tests/lm_cases.py (the ones tests/test_lm_policy_host.py runs through
lm_core.hpp, with its coverage and margin conditions) on one wave, one launch per form:

* form 1: lmw_*          -- LmState in LDS, v_readlane broadcasts;
* form 2: lmw2_*<false>  -- what k_lm runs in its 512-thread shape (row state in registers, the rest in LDS);
* form 3: lmw2_*<true>   -- what k_lm runs in its 256-thread shape (all state in registers).

Per case and form: every action, `recorded` and `evaluations` equal the reference's; last_step_norm within 1e-13,
cost within 1e-12 relative; every proposed point within the bound lm_ref.point_bound derives from the reference's own
50-digit solve: 64 eps cond2(M) max|y| scale_c per tangent component, 8 eps |x| for the quaternion product and the
series, nothing else -- in particular nothing for the policy's own previous point, from which a replayed policy steps.
Non-finite cases: actions, `recorded` and `evaluations` only.  The forms are then compared with each other and with
lm_core.hpp: same decisions, points within the sum of the two bounds.

Worst observed error / bound over all proposed points (a record of the first run on an MI355X, not a threshold):
    form 0 (lm_core.hpp, host)   0.243
    form 1                       0.122
    form 2                       0.122
    form 3                       0.122

Deliberate breaks of lm_wave.hpp, each built in a scratch copy and run through this module on an MI355X:
    `S.dec = dec` dropped under `touched`          red: forms 2 and 3, indefinite_two_invalid (last_step_norm)
    `a < 0.05` changed to `a < 0.5`                red: forms 2 and 3, first in box_turned_1.3_83 (a proposed point)
    one Newton step removed from fast_rcp          NOT detected: worst ratio 0.125 instead of 0.122 -- v_rcp_f64 with
                                                   one step is within an ulp or two already, far inside 64 eps cond2
    `reuse_diag = 0` after a rejection             cannot be detected by any test: A is unchanged after a rejection, so
                                                   the diagonal recomputed from it is the one that would be reused
"""
import numpy as np
import pytest

from tests import lm_cases, lm_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replays(lom):
    admitted, _ = lm_cases.all_cases()
    solves = [lm_cases.as_solve(c) for c in admitted]
    return admitted, {form: lom.debug_lm_policy(form, solves) for form in (0, 1, 2, 3)}


@pytest.mark.parametrize("form", (1, 2, 3))
def test_wave_form_against_the_reference(replays, form):
    admitted, got = replays
    worst = 0.0
    for c, g in zip(admitted, got[form]):
        worst = max(worst, lm_cases.check_solve(c, g, f"form {form}"))
    print(f"form {form}: worst error / bound = {worst:.3g}")
    assert worst > 0.0


def test_forms_against_each_other(replays):
    admitted, got = replays
    for a in (0, 1, 2, 3):
        for b in range(a + 1, 4):
            for c, ga, gb in zip(admitted, got[a], got[b]):
                name = (a, b, c["name"])
                assert ga["actions"] == gb["actions"], name
                assert ga["recorded"] == gb["recorded"] and ga["evaluations"] == gb["evaluations"], name
                if c["recipe"] == "nonfinite":
                    continue
                assert abs(ga["last_step_norm"] - gb["last_step_norm"]) <= 2e-13, name
                assert abs(ga["cost"] - gb["cost"]) <= 2e-12 * abs(ga["cost"]), name
                for e, pa, pb in zip(c["trace"], ga["points"], gb["points"]):
                    if e["action"] == lm_ref.LM_EVAL:
                        assert np.all(np.abs(pa - pb) <= 2.0 * e["bound"]), (name, e["tag"])


def test_replay_is_deterministic(lom, replays):
    admitted, got = replays
    again = lom.debug_lm_policy(3, [lm_cases.as_solve(c) for c in admitted])
    for ga, gb in zip(got[3], again):
        assert ga["actions"] == gb["actions"] and np.array_equal(ga["points"], gb["points"], equal_nan=True)
