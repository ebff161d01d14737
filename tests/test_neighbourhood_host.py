"""Neighbourhood classifier, the parts that need no GPU: the reference (tests/neighbourhood_ref.py) decides the scenes
of tests/test_neighbourhood_gpu.py well enough for them to be a test, the C ABI is declared in capi.py, and bad
arguments are refused before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import neighbourhood_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lom_classify_neighbourhood", "lom_frontend_set_classifier", "lom_odometry_set_classifier",
               "lom_frontend_debug_counter"]


@pytest.mark.parametrize("scene", ["room", "blob"])
def test_reference_leaves_the_scenes_well_defined(scene, oracle):
    """Conditions on the scenes, not measurements of the code: at most 2 % of the points ill-defined for count or flag,
    at most 10 % of the planar points without a stable normal (both scenes as committed: none of either)."""
    if scene == "room":
        xyz, lab = R.room_scene()
        ref = R.classify(xyz, R.ROOM_PARAMS)
    else:
        xyz = R.blob_scene()
        ref = R.classify(xyz, R.BLOB_PARAMS)
    n = len(xyz)
    print(scene, "ill count", ref["ill_count"].sum(), "ill flag", ref["ill_flag"].sum(), "planar", ref["planar"].sum(),
          "unstable normal among planar", (ref["gap"][ref["planar"]] <= R.GAP).sum())
    assert ref["ill_count"].mean() <= 0.02
    assert ref["ill_flag"].mean() <= 0.02
    planar = ref["planar"]
    if planar.any():
        assert (ref["gap"][planar] <= R.GAP).mean() <= 0.10
    if scene == "room":
        assert n > 5500
        # the scene tests what it is meant to test: walls planar, clutter and the line not, the line BECAUSE of min_spread
        assert planar[lab == 0].mean() > 0.6                                     # (a band of one radius along every edge is not)
        assert not planar[lab == 1].any()
        assert not planar[lab == 2].any() and not planar[lab == 3].any()
        line = lab == 2
        tr = ref["eig"][line].sum(1)
        assert (ref["neighbours"][line] >= R.ROOM_PARAMS["min_neighbours"]).all()
        assert (ref["eig"][line, 0] / tr <= R.ROOM_PARAMS["max_variation"]).all()  # only the spread rejects it
        assert (~ref["stored"]).sum() > 100                                         # the cap bites (clutter, line)
    else:
        assert (~ref["stored"]).sum() > 100
        assert ref["neighbours"].max() <= 27 * R.BLOB_PARAMS["index_cap"]


def test_reference_cap_semantics():
    """Ten points in one voxel with cap 4: the first four are stored, everybody's neighbours are those four, and a point
    that was not stored is not its own neighbour."""
    pts = (np.array([5.02, 1.02, 0.52]) + 0.005 * np.arange(10)[:, None]).astype(np.float32)
    ref = R.classify(pts, R.params(0.1, 4, 3, 1.0 / 3.0, 0.0))
    assert ref["stored"].tolist() == [True] * 4 + [False] * 6
    assert (ref["neighbours"] == 4).all()


def test_new_symbols_are_declared(lom):
    text = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lom.capi.EXPORTED, name
        assert getattr(lom.capi.lib(), name).argtypes is not None, name
    assert re.search(r"#define\s+LOM_ABI_VERSION\s+2\b", text)
    assert lom.capi.NEIGHBOURHOOD_DETAIL.itemsize == 32 and C.sizeof(lom.capi.NeighbourhoodParams) == 20
    assert (lom.capi.CLASSIFIER_RINGS, lom.capi.CLASSIFIER_NEIGHBOURHOOD) == (0, 1)


def test_bad_arguments_are_refused(lom):
    L, ERR_ARG = lom.capi.lib(), lom.capi.ERR_ARG
    good = lom.neighbourhoodParams(R.ROOM_PARAMS)
    assert L.lom_odometry_set_classifier(None, 1, C.byref(good)) == ERR_ARG
    assert L.lom_odometry_set_classifier(None, 0, None) == ERR_ARG
    assert L.lom_frontend_set_classifier(None, 1, C.byref(good)) == ERR_ARG
    assert L.lom_classify_neighbourhood(None, None, 0, C.byref(good), None, None, None) == ERR_ARG
    assert L.lom_frontend_debug_counter(None, 0) == ERR_ARG
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(index_cap=0),
           dict(index_cap=65), dict(min_neighbours=2), dict(max_variation=0.0), dict(max_variation=0.34),
           dict(max_variation=float("nan")), dict(min_spread=-0.1), dict(min_spread=1.0), dict(min_spread=float("nan"))]
    for change in bad:
        p = lom.neighbourhoodParams(dict(R.ROOM_PARAMS, **change))
        assert L.lom_odometry_set_classifier(None, 1, C.byref(p)) == ERR_ARG, change
        assert L.lom_frontend_set_classifier(None, 1, C.byref(p)) == ERR_ARG, change
    with pytest.raises(TypeError):
        lom.neighbourhoodParams(dict(radius=0.5))  # no defaults: all five fields or none
