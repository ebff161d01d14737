"""Batched align (lom_match_align_batch): what runs without a GPU -- the entry points load, argument errors are found
before any device is touched, and the best-result rule of lom_align_batch_best."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def capi(lom):
    return lom.capi


def _results(capi, rows):
    """rows: [(valid_last, final_cost), ...] -> lom_align_result array"""
    r = (capi.AlignResult * max(len(rows), 1))()
    for i, (valid, cost) in enumerate(rows):
        r[i].stats.valid_last = valid
        r[i].stats.final_cost = cost
    return r


def test_batch_symbols_load(capi):
    L = capi.lib()
    for name in ("lom_match_align_batch", "lom_match_align_batch_device", "lom_scan_align_batch",
                 "lom_scan_align_batch_device", "lom_align_batch_best"):
        assert name in capi.EXPORTED
        assert hasattr(L, name)
    assert capi.OPT_TEST_BATCH_ROUND_MAX == 107


@pytest.mark.parametrize("name", ["lom_match_align_batch", "lom_match_align_batch_device", "lom_scan_align_batch",
                                  "lom_scan_align_batch_device"])
def test_batch_argument_errors(capi, name):
    fn = getattr(capi.lib(), name)
    probs = (capi.AlignProblem * 2)()
    res = (capi.AlignResult * 2)()
    best = C.c_int(7)
    # NULL map / context, whatever else is given
    assert fn(None, probs, 2, res, C.byref(best)) == -1
    assert fn(None, probs, 0, res, None) == -1
    assert fn(None, None, 0, None, None) == -1
    assert fn(None, probs, -1, res, None) == -1
    assert fn(None, None, 2, res, None) == -1
    assert fn(None, probs, 2, None, None) == -1
    assert best.value == 7  # untouched on an argument error


def test_best_most_valid_wins(capi):
    r = _results(capi, [(10, 1.0), (30, 5.0), (20, 0.1)])
    assert capi.lib().lom_align_batch_best(r, 3) == 1


def test_best_tie_on_valid_goes_to_lower_cost(capi):
    r = _results(capi, [(30, 2.0), (30, 1.5), (10, 0.0), (30, 1.75)])
    assert capi.lib().lom_align_batch_best(r, 4) == 1


def test_best_tie_on_both_goes_to_lower_index(capi):
    r = _results(capi, [(5, 9.0), (30, 1.5), (30, 1.5), (30, 1.5)])
    assert capi.lib().lom_align_batch_best(r, 4) == 1
    r = _results(capi, [(0, 0.0), (0, 0.0)])
    assert capi.lib().lom_align_batch_best(r, 2) == 0


def test_best_of_nothing(capi):
    r = _results(capi, [])
    assert capi.lib().lom_align_batch_best(r, 0) == -1
    assert capi.lib().lom_align_batch_best(None, 0) == -1
    assert capi.lib().lom_align_batch_best(r, -3) == -1


def test_python_mirror_has_batch_entry(lom):
    m = lom.CloudMatcher()
    assert hasattr(m, "alignBatch") and hasattr(m, "alignBatchDevice")
    assert m.batch_stats is None and m.best is None
