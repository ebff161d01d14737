"""Multi-map align (lom_match_align_multi) and batched odometry (lom_odometry_process_batch): what runs without a GPU --
the entry points load, argument errors are found before any device is touched, and the Python mirrors exist."""
import ctypes as C

import pytest

NAMES = ("lom_match_align_multi", "lom_match_align_multi_device", "lom_odometry_process_batch")


@pytest.fixture(scope="module")
def capi(lom):
    return lom.capi


def test_multi_symbols_load(capi):
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTED
        assert hasattr(L, name)
    assert L.lom_abi_version() == 2
    # the problem descriptor: the map handle, then lom_align_problem's fields
    assert capi.AlignMultiProblem.map.offset == 0 and capi.AlignMultiProblem.xyz.offset == 8
    assert C.sizeof(capi.AlignMultiProblem) == 8 + C.sizeof(capi.AlignProblem)


@pytest.mark.parametrize("name", ["lom_match_align_multi", "lom_match_align_multi_device"])
def test_multi_argument_errors(capi, name):
    fn = getattr(capi.lib(), name)
    probs = (capi.AlignMultiProblem * 2)()
    res = (capi.AlignResult * 2)()
    best = C.c_int(7)
    # NULL runner, whatever else is given (NULL problem maps too)
    assert fn(None, probs, 2, res, C.byref(best)) == capi.ERR_ARG
    assert fn(None, probs, 0, res, C.byref(best)) == capi.ERR_ARG
    assert fn(None, None, 0, None, None) == capi.ERR_ARG
    assert fn(None, probs, -1, res, C.byref(best)) == capi.ERR_ARG
    assert fn(None, None, 2, res, C.byref(best)) == capi.ERR_ARG
    assert fn(None, probs, 2, None, C.byref(best)) == capi.ERR_ARG
    assert best.value == 7  # untouched on an argument error


def test_process_batch_argument_errors(capi):
    L = capi.lib()
    hs = (C.c_void_p * 2)(None, None)
    frames = (C.c_void_p * 2)(None, None)
    ns = (C.c_size_t * 2)(0, 0)
    st = (C.c_int * 2)(5, 5)
    assert L.lom_odometry_process_batch(hs, frames, ns, -1, st) == capi.ERR_ARG
    assert L.lom_odometry_process_batch(None, frames, ns, 2, st) == capi.ERR_ARG
    assert L.lom_odometry_process_batch(hs, None, ns, 2, st) == capi.ERR_ARG
    assert L.lom_odometry_process_batch(hs, frames, None, 2, st) == capi.ERR_ARG
    assert L.lom_odometry_process_batch(hs, frames, ns, 2, st) == capi.ERR_ARG  # NULL handles
    assert list(st) == [5, 5]  # refused before any stream: no status written
    # nothing to do is not an error
    assert L.lom_odometry_process_batch(None, None, None, 0, None) == capi.OK


def test_python_mirrors_exist(lom):
    assert callable(lom.CloudMatcher.alignMulti)
    assert callable(lom.CloudMatcher.alignMultiDevice)
    assert callable(lom.LidarOdometry.processBatch)
    assert lom.LidarOdometry.processBatch([], []) is None
    with pytest.raises(ValueError):
        lom.CloudMatcher().alignMulti([], [None], [])
    with pytest.raises(ValueError):
        lom.LidarOdometry.processBatch([], [None])
