"""Rows f2 / f3 (deskew, classifier, filters) against an INDEPENDENT restatement of the reference text.

oracle/pipeline.c and the product's host stages (csrc/host_stages.cpp) share their text, and the device front end is
compared with that same oracle: a misreading of src/utils/*.h common to both would pass every such test.
tests/restate_frontend.py restates the four stages in numpy straight from the reference's headers; its output for
three seeded frames is pinned by digests in tests/golden/frontend_restated.npz (make_frontend_fixtures.py).  Here:

* the live restatement still reproduces the committed digests (CPU);
* the oracle's chain equals it, array by array, bit for bit (CPU);
* the product's host stages and the device front end equal it (GPU);
* every alternative READING of the C++ text the restatement implements (double vs float atan2 / sqrt overloads, the
  evaluation order of Eigen's 4-vector dot product) is quantified: how many planar points of a frame it moves.
The reference holds no vector for these stages: parity with the reference itself stays unpinned."""
import os

import numpy as np
import pytest

from lidar_odometry_demo_amd import synth
from tests import restate_frontend as R
from tests.conftest import GOLDEN
from tests.golden.make_frontend_fixtures import CASES, DIGESTED, digest

IDENT = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))


@pytest.fixture(scope="module")
def restated():
    fx = np.load(os.path.join(GOLDEN, "frontend_restated.npz"))
    out = []
    for i, (k, (st, sq)) in enumerate(CASES):
        frame = synth.make_sequence_frame(k)
        out.append((frame, (st, sq), R.front_end(frame, st, sq, *IDENT), {key[len(f"f{i}_"):]: fx[key] for key in fx.files
                                                                            if key.startswith(f"f{i}_")}))
    return out


def test_restatement_reproduces_the_committed_fixture(restated):
    for frame, _, got, fx in restated:
        assert tuple(got["shape"]) == tuple(fx["shape"])
        assert [len(frame), len(got["planar_cell"]), int(got["kept"].sum())] == list(fx["counts"])
        assert [digest(got[k]) for k in DIGESTED] == list(fx["digests"])
        assert np.array_equal(got["planar_cell"][::16], fx["sample_cell"])
        assert got["planar_nrm"][::16].tobytes() == fx["sample_nrm"].tobytes()


def test_readings_of_the_cpp_text_are_quantified(restated):
    """double vs float atan2 (cloud_classifier.h:49), double vs float sqrt (:97), the order of Eigen's quaternion dot
    product: recorded per frame as (planar cells that differ, shared cells whose normal moves by > 1e-6, planar cells).
    On frames with vehicle motion none of them moves a single planar point; on a frame deskewed with the identity the
    synthetic azimuths sit exactly on the bin boundaries and the atan2 reading decides the cell of a third of them --
    the case the device front end hands back to the host (`redo_on_host`)."""
    for i, (_, _, _, fx) in enumerate(restated):
        r = fx["readings"]
        assert r.shape == (3, 3)
        if i < 2:
            assert (r[:, 0] == 0).all() and (r[:, 1] <= 5).all(), (i, r)
        assert (r[1:, 0] == 0).all() and (r[1:, 1] == 0).all(), (i, r)   # sqrt overload, dot order: nothing moves


def _oracle_chain(oracle, frame, start):
    desk = oracle.transformNonRigid(oracle.pointTimeNormalize(frame), oracle.Pose3D(*start), oracle.Pose3D(*IDENT))
    xyz, nrm, _, grid = oracle.classify(desk)
    fxyz, fnrm = oracle.rangeFilter(xyz, nrm, 4.0, 80.0)
    return desk, xyz, nrm, fxyz, fnrm, grid


def _assert_equals_restatement(got, desk, xyz, nrm, fxyz, fnrm, grid):
    assert np.stack([desk["x"], desk["y"], desk["z"]], 1).tobytes() == got["deskewed_xyz"].tobytes()
    assert tuple(grid) == tuple(got["shape"])
    assert len(xyz) == len(got["planar_cell"])
    assert xyz.tobytes() == got["planar_xyz"].tobytes()
    assert nrm.tobytes() == got["planar_nrm"].tobytes()
    keep = got["kept"]
    assert fxyz.tobytes() == got["planar_xyz"][keep].tobytes() and fnrm.tobytes() == got["planar_nrm"][keep].tobytes()


def test_oracle_chain_equals_the_independent_restatement(oracle, restated):
    for frame, start, got, _ in restated:
        _assert_equals_restatement(got, *_oracle_chain(oracle, frame, start))


@pytest.mark.gpu
def test_host_stages_and_device_front_end_equal_the_independent_restatement(lom, restated):
    fe = lom.FrontEnd()
    for i, (frame, start, got, _) in enumerate(restated):
        desk = lom.transformNonRigid(lom.pointTimeNormalize(frame), lom.Pose3D(*start), lom.Pose3D(*IDENT))
        xyz, nrm, _, grid = lom.classify(desk)
        fxyz, fnrm = lom.rangeFilter(xyz, nrm, 4.0, 80.0)
        _assert_equals_restatement(got, desk, xyz, nrm, fxyz, fnrm, grid)
        dev = fe.process(frame, lom.Pose3D(*start), lom.Pose3D(*IDENT), 4.0, 80.0)
        if dev["redo_on_host"]:
            assert i == 2        # azimuths on the bin boundaries: the device hands the frame back (see above)
            continue
        keep = got["kept"]
        dd = dev["deskewed"]
        assert np.stack([dd["x"], dd["y"], dd["z"]], 1).tobytes() == got["deskewed_xyz"].tobytes()
        assert tuple(dev["grid"]) == tuple(got["shape"]) and dev["planar_points"] == len(got["planar_cell"])
        assert dev["xyz"].tobytes() == got["planar_xyz"][keep].tobytes()
        assert dev["normals"].tobytes() == got["planar_nrm"][keep].tobytes()
