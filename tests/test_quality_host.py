"""Host side of the align quality report, without a GPU: the new C ABI symbols and the layout of lom_quality_report,
and lom_quality_from_sums (csrc/quality.cpp) on reduced sums that come from the ORACLE -- Shard.match_eval's 28 sums and
the values beyond them restated in numpy from the oracle's correspondences (tests/quality_ref.py).

Bars (the reference side is numpy.linalg on the same sums):
* information: the sums, mirrored, bit for bit (it is a copy);
* eigenvalues within 1e-9 * ||block||_F of numpy.linalg.eigvalsh -- Weyl bounds an eigenvalue's change by the norm of
  the input difference, and Jacobi's own round-off is a few ulp (1e-16) of the norm: three orders of margin and more;
* eigenvectors by residual, ||A v - lambda v|| <= 1e-9 ||A||: independent of sign and of the order of close eigenvalues;
* covariance against sigma2 * inv(S P H P^T S) by numpy to a relative 1e-10 * cond, cond computed here from the oracle's
  matrix and asserted < 1e8 first, so that the tolerance stays below 1e-2 and means something."""
import ctypes as C

import numpy as np
import pytest

from tests import quality_ref as Q
from tests import scenes

NEW_SYMBOLS = ["lom_quality_from_sums", "lom_match_quality", "lom_match_quality_device", "lom_scan_quality",
               "lom_scan_quality_device", "lom_odometry_set_quality_thresholds", "lom_odometry_get_quality"]


def test_symbols_and_struct_layout(lom):
    L = lom.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in lom.capi.EXPORTED, name
        assert hasattr(L, name), name
    assert lom.capi.OPT_QUALITY_REPORT == 8 and lom.capi.NQSUMS == 36
    R = lom.capi.QualityReport
    assert C.sizeof(R) == Q.REPORT_SIZE
    assert [(k, getattr(R, k).offset, getattr(R, k).size) for k, _ in R._fields_] == Q.REPORT_LAYOUT
    assert L.lom_abi_version() == 2


def _oracle_sums(oracle, og, scan, pose_t, pose_q):
    """LOM_NQSUMS values at the f32 pose widened to f64, all from the oracle; also (valid, r) per point."""
    pose = oracle.Pose3D(pose_t, pose_q)
    q, t = pose.rotation.astype(np.float64), pose.translation.astype(np.float64)
    ref = oracle.Shard(og, scan).match_eval(pose.translation, pose.rotation, q, t)
    pairs = og.findMatchingPairs(scan, pose, 0.3)
    valid, r, d2 = Q.residuals_from_pairs(pairs, scan, q, t)
    assert int(valid.sum()) == int(ref[28])
    return Q.sums36(ref, Q.extra_sums(valid, r, d2)), valid, r


def _check_against_numpy(lom, sums, queries, tag):
    rep = Q.from_sums(lom, sums, queries)
    H = Q.full_information(sums)
    assert rep["information"].tobytes() == H.tobytes(), tag
    assert rep["gradient"].tobytes() == np.asarray(sums[21:27]).tobytes(), tag
    valid = int(sums[33])
    assert (rep["queries"], rep["valid"], rep["inliers"]) == (queries, valid, int(sums[34])), tag
    assert rep["overlap"] == valid / queries and rep["cost"] == sums[27] and rep["sum_w"] == sums[28]
    assert rep["max_abs_residual"] == sums[35]
    for got, want in ((rep["rmse"], np.sqrt(sums[30] / valid)), (rep["rmse_inliers"], np.sqrt(sums[31] / sums[34])),
                      (rep["mean_sq_dist"], sums[32] / valid), (rep["sigma2"], sums[29] / max(1, valid - 6))):
        assert abs(got - want) <= 4 * np.finfo(np.float64).eps * abs(want), (tag, got, want)
    for block, w, V in ((H[3:, 3:] / sums[28], rep["eig_t"], rep["eigvec_t"]),
                        (H[:3, :3] / (4.0 * sums[28]), rep["eig_r"], rep["eigvec_r"])):
        norm = np.linalg.norm(block)
        assert np.all(np.diff(w) >= 0), (tag, w)
        assert np.abs(w - np.linalg.eigvalsh(block)).max() <= 1e-9 * norm, (tag, w)
        for k in range(3):
            v = V[k]
            assert abs(np.linalg.norm(v) - 1.0) < 1e-12
            assert np.linalg.norm(block @ v - w[k] * v) <= 1e-9 * norm, (tag, k)
    assert abs(rep["eig_t"].sum() - 1.0) < 1e-6, (tag, rep["eig_t"])   # f32 unit normals: trace of the mean n n^T
    M = Q.nav_information(H)
    cond = np.linalg.cond(M)
    assert cond < 1e8, (tag, cond)
    ref_cov = rep["sigma2"] * np.linalg.inv(M)
    assert rep["covariance_valid"] == 1, tag
    err = np.linalg.norm(rep["covariance"] - ref_cov) / np.linalg.norm(ref_cov)
    print(f"{tag}: valid {valid} cond {cond:.3e} covariance rel err {err:.3e} eig_t {rep['eig_t']} eig_r {rep['eig_r']}")
    assert err <= 1e-10 * cond, (tag, err, cond)
    assert np.array_equal(rep["covariance"], rep["covariance"].T)
    return rep


POSES = [((0, 0, 0), (1, 0, 0, 0)),
         ((0.05, -0.04, 0.03), scenes.angle_axis_q(0.004, (0, 0, 1))),
         # f32, NOT renormalised: a pose as it stands between two outer iterations; |r| on both sides of the Huber knee
         ((0.1, -0.1, 0.1), np.array([0.99993, 0.0031, -0.0042, 0.0105], np.float32))]


def test_from_sums_small_synth_vs_numpy(lom, oracle):
    sm = scenes.small_synth_case()
    og = oracle.VoxelGrid(0.5, 20)
    og.addCloud(sm["map_xyz"], sm["map_nrm"])
    outliers = 0
    for i, (t, q) in enumerate(POSES):
        sums, valid, r = _oracle_sums(oracle, og, sm["scan"], t, q)
        rep = _check_against_numpy(lom, sums, len(sm["scan"]), ("synth", i))
        outliers += rep["valid"] - rep["inliers"]
    assert outliers > 0   # the Huber branch took part


def test_from_sums_fixture_c1_vs_numpy(lom, oracle, fixture_cloud):
    xyz, xyzn = fixture_cloud
    og = oracle.VoxelGrid(0.25, 20)
    og.addCloud(xyzn[:, :3], xyzn[:, 3:])
    vf = oracle.VoxelGrid(0.5, 1)
    vf.addCloudWithoutNormals(xyz)
    scan = vf.getCloudWithoutNormals()
    for i, (t, q) in enumerate(POSES):
        sums, valid, r = _oracle_sums(oracle, og, scan, t, q)
        _check_against_numpy(lom, sums, len(scan), ("C1", i))


def test_degenerate_corridor_and_corner(lom, oracle):
    """A corridor along x constrains nothing along x: the smallest share is exactly 0, along +-x, the factorisation
    meets a zero pivot.  With an end wall every direction is constrained."""
    xyz, nrm, scan = Q.corridor_scene()
    og = oracle.VoxelGrid(0.5, 20)
    og.addCloud(xyz, nrm)
    sums, valid, r = _oracle_sums(oracle, og, scan, (0, 0, 0), (1, 0, 0, 0))
    assert valid.all() and not np.nan_to_num(r).any()           # the scan is a subset of the map
    second = np.linalg.eigvalsh(Q.full_information(sums)[3:, 3:] / sums[28])[1]
    assert second > 0.1
    for thr in (0.5 * second, 1e-3, 1e-30):
        rep = Q.from_sums(lom, sums, len(scan), thr, 0.0)
        assert rep["eig_t"][0] == 0.0
        assert np.abs(rep["eigvec_t"][0]).tolist() == [1.0, 0.0, 0.0]
        assert rep["degenerate_t"] == 1 and rep["degenerate_r"] == 0, thr
        assert rep["covariance_valid"] == 0 and not rep["covariance"].any()
    xyz, nrm, scan = Q.corridor_scene(end_wall=True)
    og = oracle.VoxelGrid(0.5, 20)
    og.addCloud(xyz, nrm)
    sums, valid, r = _oracle_sums(oracle, og, scan, (0, 0, 0), (1, 0, 0, 0))
    smallest = np.linalg.eigvalsh(Q.full_information(sums)[3:, 3:] / sums[28])[0]
    assert smallest > 1e-3
    rep = Q.from_sums(lom, sums, len(scan), 1e-3, 1e-3)
    assert rep["degenerate_t"] == 0 and rep["degenerate_r"] == 0 and rep["covariance_valid"] == 1
    assert rep["eig_t"][0] > 1e-3


def _spd_sums(valid):
    """sums of `valid` synthetic unit-weight correspondences with a well-conditioned H."""
    rng = np.random.default_rng(3)
    J = rng.normal(size=(max(valid, 12), 6))
    H = J.T @ J
    s = np.zeros(36)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            s[k] = H[a, b]
            k += 1
    s[28], s[29], s[30], s[31], s[32], s[33], s[34], s[35] = valid, 0.02, 0.02, 0.02, 0.5, valid, valid, 0.1
    return s


def test_edge_cases(lom):
    L = lom.capi.lib()
    rep = Q.from_sums(lom, np.zeros(36), 100, 0.1, 0.1)          # no correspondence at all
    assert (rep["queries"], rep["valid"], rep["overlap"], rep["covariance_valid"]) == (100, 0, 0.0, 0)
    assert rep["rmse"] == 0.0 and rep["sigma2"] == 0.0 and not rep["eig_t"].any() and not rep["covariance"].any()
    assert rep["degenerate_t"] == 3 and rep["degenerate_r"] == 3  # nothing is constrained
    rep = Q.from_sums(lom, np.zeros(36), 0)                      # no query: overlap 0, thresholds off
    assert rep["overlap"] == 0.0 and rep["degenerate_t"] == 0 and rep["degenerate_r"] == 0
    six, seven = Q.from_sums(lom, _spd_sums(6), 10), Q.from_sums(lom, _spd_sums(7), 10)
    assert six["covariance_valid"] == 0 and not six["covariance"].any() and six["sigma2"] == 0.02
    assert seven["covariance_valid"] == 1 and seven["sigma2"] == 0.02
    assert np.allclose(seven["covariance"], 0.02 * np.linalg.inv(Q.nav_information(Q.full_information(_spd_sums(7)))),
                       rtol=1e-9, atol=0)
    for thr in (0.0, -1.0):                                      # thresholds <= 0: not counted
        rep = Q.from_sums(lom, np.zeros(36), 100, thr, thr)
        assert rep["degenerate_t"] == 0 and rep["degenerate_r"] == 0
    for slot, bad in ((0, np.nan), (20, np.inf), (29, np.nan), (29, np.inf)):   # non-finite H or sigma2: no covariance
        s = _spd_sums(50)
        s[slot] = bad
        rep = Q.from_sums(lom, s, 60, 0.1, 0.1)
        assert rep["covariance_valid"] == 0 and not rep["covariance"].any(), (slot, bad)
        if slot == 0:    # the rotation block is not finite: no spectrum, no count; the translation block has one
            assert np.isnan(rep["eig_r"]).all() and rep["degenerate_r"] == 0 and np.isfinite(rep["eig_t"]).all()
    for bad in (np.nan, np.inf):                                 # non-finite sum of weights: no spectra, no counts
        s = _spd_sums(50)
        s[28] = bad
        rep = Q.from_sums(lom, s, 60, 0.1, 0.1)
        assert np.isnan(rep["eig_t"]).all() and np.isnan(rep["eig_r"]).all()
        assert rep["degenerate_t"] == 0 and rep["degenerate_r"] == 0
    rep = lom.capi.QualityReport()
    arr = (C.c_double * 36)()
    assert L.lom_quality_from_sums(None, 1, 0.0, 0.0, C.byref(rep)) == lom.capi.ERR_ARG
    assert L.lom_quality_from_sums(arr, 1, 0.0, 0.0, None) == lom.capi.ERR_ARG
    assert L.lom_quality_from_sums(arr, -1, 0.0, 0.0, C.byref(rep)) == lom.capi.ERR_ARG
