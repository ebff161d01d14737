"""The pose graph on the device (lom_graph_*, csrc/k_graph.hpp) against the numpy reference tests/graph_ref.py: the
linearisation and the mat-vec entry by entry within graph_ref.REL of each entry's sum of absolute terms, the optimum judged
by the reference (its own gradient at the device's answer, its own optimum within the pose-parity bar), exact recovery, a
false closure, determinism, incremental use, the refusals on a live graph, and the chain from an align to an edge.
Shapes: one node; one edge; one past a wave (65) and one past a workgroup (257); a 600-node graph with a hub of degree 200
on the fixed node and a second hub on a free node (the 16-lane rows of the node kernels); duplicate edges; a second fixed
node in the middle.  Measured distances to the reference's optimum: profiles/graph_parity.json."""
import numpy as np
import pytest

from tests import graph_cases as gc
from tests import graph_ref as ref
from tests import scenes

pytestmark = pytest.mark.gpu
REL = ref.REL


def _within(got, want, scale, what):
    err = np.abs(np.asarray(got) - np.asarray(want))
    bar = REL * np.asarray(scale)
    worst = float((err / np.maximum(bar, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst error / bar = {worst:.3g}")
    assert np.all(err <= bar), (what, worst)


def _check_evaluate(lom, graph, poses, lam):
    pg = gc.build(lom, graph, poses)
    lin = ref.linearise(graph, poses, lam)
    ev = pg.evaluate(lam)
    assert np.array_equal(ev["w"] < 1.0, lin["w"] < 1.0), "an edge took the other Huber branch"
    _within(ev["e"], lin["e"], lin["e_abs"], "e")
    _within(pg.chi2(), lin["s"], lin["s_abs"], "s")
    # w = delta / sqrt(s) carries half of s's relative error (and is exactly 1 on the plain branch)
    _within(ev["w"], lin["w"], lin["w"] * (1.0 + 0.5 * lin["s_abs"] / np.maximum(lin["s"], 1e-300)), "w")
    _within(ev["cost"], lin["cost"], lin["cost_abs"], "cost")
    _within(ev["g"], lin["g"], lin["g_abs"], "g")
    _within(ev["hdiag"], lin["hdiag"], lin["hdiag_abs"], "hdiag")
    fixed = np.asarray(graph["fixed"], bool)
    assert not ev["g"][fixed].any() and not ev["hdiag"][fixed].any()
    return pg, lin


@pytest.mark.parametrize("name", gc.CASES)
@pytest.mark.parametrize("huber", [False, True], ids=["plain", "huber"])
def test_evaluate_at_the_guess_and_at_the_optimum(lom, name, huber):
    graph, _ = gc.case(name)
    for poses, lam in ((graph["poses"], 0.0), (gc.optimum(name)[0], 0.37)):
        g = gc.with_huber(graph, poses) if huber and len(graph["ij"]) >= 3 else graph
        if huber and len(graph["ij"]) >= 3:
            share = (ref.linearise(g, poses)["w"] < 1).mean()
            assert 0.2 < share < 0.45
        _check_evaluate(lom, g, poses, lam)


@pytest.mark.parametrize("name", gc.CASES)
def test_matvec(lom, name):
    graph, _ = gc.case(name)
    pg = gc.build(lom, graph)
    rng = np.random.default_rng(5)
    fixed = np.asarray(graph["fixed"], bool)
    for lam in (0.0, 2.5):
        lin = ref.linearise(graph, None, lam)
        for _ in range(3):
            p = rng.normal(size=(len(fixed), 6))
            y, y_abs = ref.matvec(graph, lin, lam, p)
            got = pg.matvec(lam, p)
            _within(got, y, y_abs, f"y lambda={lam}")
            assert not got[fixed].any()


def _check_optimum(graph, pg, st, want_poses, before):
    """before: the poses the graph held on entry (quaternions as normalised by the graph)"""
    got = pg.poses()
    lin = ref.linearise(graph, got)
    gmax = float(np.abs(lin["g"]).max())
    print("reference gradient at the device's answer:", gmax, "stats:", st)
    assert gmax <= gc.PARAMS["gtol"]
    assert st["stop_reason"] == lom_stop_gradient()
    _within(st["cost_final"], lin["cost"], lin["cost_abs"], "cost_final")
    assert st["pcg_capped"] == 0 and st["outer"] <= gc.PARAMS["max_outer"]
    dt, dr = ref.pose_delta(got, want_poses)
    print(f"distance to the reference's optimum: {dt:.3e} m {dr:.3e} rad")
    assert dt < gc.POSE_BAR and dr < gc.POSE_BAR
    fixed = np.asarray(graph["fixed"], bool)
    assert got[fixed].tobytes() == before[fixed].tobytes()
    return dt, dr


def lom_stop_gradient():
    import lidar_odometry_demo_amd as pkg

    return pkg.capi.GRAPH_STOP_GRADIENT


@pytest.mark.parametrize("name", gc.CASES)
def test_optimum(lom, name):
    graph, _ = gc.case(name)
    pg = gc.build(lom, graph)
    before = pg.poses()
    st = pg.optimize(gc.PARAMS)
    _check_optimum(graph, pg, st, gc.optimum(name)[0], before)
    assert st["cost_initial"] == pytest.approx(ref.linearise(graph)["cost"], rel=1e-9)


def test_one_fixed_node_and_no_edge(lom):
    graph, _ = gc.case("n1")
    pg = gc.build(lom, graph)
    before = pg.poses()
    assert ref.pose_delta(before, graph["poses"]) < (1e-15, 1e-7)  # (the quaternion is normalised on entry)
    st = pg.optimize(gc.PARAMS)
    assert st["outer"] == 0 and st["cost_final"] == 0.0 and st["stop_reason"] == lom.capi.GRAPH_STOP_GRADIENT
    assert pg.poses().tobytes() == before.tobytes() and pg.evaluate()["cost"] == 0.0 and len(pg.chi2()) == 0


def test_exact_recovery(lom):
    graph, truth = gc.case("n65_exact")
    pg = gc.build(lom, graph)
    st = pg.optimize(gc.PARAMS)
    dt, dr = ref.pose_delta(pg.poses(), truth)
    print(f"distance to the ground truth: {dt:.3e} m {dr:.3e} rad; cost {st['cost_initial']:.3e} -> {st['cost_final']:.3e}")
    assert dt < gc.POSE_BAR and dr < gc.POSE_BAR
    assert st["cost_final"] < 1e-12 * st["cost_initial"]


def test_false_closure(lom):
    clean, _ = gc.case("n65")
    m = len(clean["ij"])
    zbad = ref.compose(ref.between(*gc.optimum("n65")[0][[10, 40]])[None], np.array([[5.0, 0, 0, 1, 0, 0, 0]]))

    def with_bad(delta):
        return dict(clean, ij=np.concatenate([clean["ij"], np.array([[10, 40]], np.int32)]), Z=np.concatenate([clean["Z"], zbad]),
                    Om=np.concatenate([clean["Om"], clean["Om"][:1]]), delta=np.concatenate([clean["delta"], [delta]]))

    robust = gc.build(lom, with_bad(3.0))
    st_robust = robust.optimize(gc.PARAMS)
    chi2 = robust.chi2()
    assert int(np.argmax(chi2)) == m
    keep = np.arange(m + 1) != int(np.argmax(chi2))
    g = with_bad(3.0)
    rebuilt = dict(g, ij=g["ij"][keep], Z=g["Z"][keep], Om=g["Om"][keep], delta=g["delta"][keep])
    pg = gc.build(lom, rebuilt)
    before = pg.poses()
    _check_optimum(rebuilt, pg, pg.optimize(gc.PARAMS), gc.optimum("n65")[0], before)
    plain = gc.build(lom, with_bad(0.0))
    st_plain = plain.optimize(gc.PARAMS)
    print("final cost with delta = 3:", st_robust["cost_final"], "with delta = 0:", st_plain["cost_final"])
    assert st_plain["cost_final"] > st_robust["cost_final"]


def test_determinism_bulk_and_growth(lom):
    graph, _ = gc.case("n65")
    results = []
    for bulk, hints in ((True, (0, 0)), (True, (0, 0)), (False, (0, 0)), (True, (1000, 2000)), (False, (3, 2))):
        pg = gc.build(lom, graph, bulk=bulk, hints=hints)
        st = pg.optimize(gc.PARAMS)
        results.append((pg.poses().tobytes(), tuple(sorted(st.items())), pg.chi2().tobytes()))
    assert all(r == results[0] for r in results[1:])


def test_incremental_use(lom):
    graph, truth = gc.case("n65")
    n0 = 60
    first = graph["ij"].max(axis=1) < n0
    part = dict(graph, poses=graph["poses"][:n0], fixed=graph["fixed"][:n0], ij=graph["ij"][first], Z=graph["Z"][first],
                Om=graph["Om"][first], delta=graph["delta"][first])
    pg = gc.build(lom, part)
    pg.optimize(gc.PARAMS)
    mid = pg.poses()
    tail = [mid[-1]]
    for k in range(n0, 65):  # five nodes dead-reckoned from the optimised ones, then every remaining edge (the closure among them)
        tail.append(ref.compose(tail[-1], graph["Z"][k - 1]))
    assert pg.addNodes(np.array(tail[1:]), np.zeros(5, bool)) == n0
    pg.addEdges(graph["ij"][~first], graph["Z"][~first], graph["Om"][~first], graph["delta"][~first])
    st = pg.optimize(gc.PARAMS)
    order = np.concatenate([np.flatnonzero(first), np.flatnonzero(~first)])
    whole = dict(graph, poses=np.concatenate([mid, np.array(tail[1:])]), ij=graph["ij"][order], Z=graph["Z"][order],
                 Om=graph["Om"][order], delta=graph["delta"][order])
    fresh = gc.build(lom, whole)
    fresh_before = fresh.poses()
    st_fresh = fresh.optimize(gc.PARAMS)
    # (not the same bytes: the fresh graph normalises the optimised quaternions once more on entry)
    want = ref.lm(whole, gc.PARAMS)[0]
    _check_optimum(whole, pg, st, want, whole["poses"])
    _check_optimum(whole, fresh, st_fresh, want, fresh_before)
    dt, dr = ref.pose_delta(pg.poses(), fresh.poses())
    assert dt < gc.POSE_BAR and dr < gc.POSE_BAR


def test_refusals_on_a_live_graph(lom):
    graph, _ = gc.case("n7_duplicates")
    pg = gc.build(lom, graph)
    before = pg.poses().tobytes()
    E = lom.capi.ERR_ARG
    z, om = graph["Z"][0], graph["Om"][0]
    bad_om = om.copy()
    bad_om[2, 2] = -1.0
    nan_om = om.copy()
    nan_om[0, 1] = nan_om[1, 0] = np.nan
    for args in ((0, 7, z, om, 0.0), (-1, 2, z, om, 0.0), (3, 3, z, om, 0.0), (0, 1, z, bad_om, 0.0), (0, 1, z, nan_om, 0.0),
                 (0, 1, z, om, -1.0), (0, 1, z, om, np.nan), (0, 1, np.zeros(7), om, 0.0)):
        with pytest.raises(lom.LomError) as e:
            pg.addEdge(*args)
        assert e.value.code == E
    with pytest.raises(lom.LomError) as e:
        pg.addNode(np.array([0, 0, np.inf, 1, 0, 0, 0]))
    assert e.value.code == E
    assert pg.edgeCount() == len(graph["ij"]) and pg.nodeCount() == 7
    for bad in (dict(gtol=0.0), dict(lambda0=np.nan), dict(max_pcg=0), dict(max_outer=-1), dict(xtol=np.inf)):
        with pytest.raises(lom.LomError) as e:
            pg.optimize(dict(gc.PARAMS, **bad))
        assert e.value.code == E
    free = pg.addNodes(np.array([[1.0, 2, 3, 1, 0, 0, 0], [2.0, 2, 3, 1, 0, 0, 0]]), [False, False])
    pg.addEdge(free, free + 1, z, om, 0.0)  # a component without a fixed node
    with pytest.raises(lom.LomError) as e:
        pg.optimize(gc.PARAMS)
    assert e.value.code == E and f"node {free}" in str(e.value)
    assert pg.poses(0, 7).tobytes() == before
    pg.setFixed(free, True)  # usable afterwards
    st = pg.optimize(gc.PARAMS)
    assert st["stop_reason"] == lom.capi.GRAPH_STOP_GRADIENT
    dt, dr = ref.pose_delta(pg.poses(0, 7), gc.optimum("n7_duplicates")[0])
    assert dt < gc.POSE_BAR and dr < gc.POSE_BAR


def test_chain_from_align_to_edge(lom):
    """align -> quality -> information_from_quality -> add_edge: two scans against one keyframe, a 3-node graph"""
    case = scenes.small_synth_case()
    grid = lom.VoxelGrid(0.5, 20)
    grid.addCloud(case["map_xyz"], case["map_nrm"])
    matcher = lom.CloudMatcher()
    pg = lom.PoseGraph()
    ident = np.array([0.0, 0, 0, 1, 0, 0, 0])
    assert pg.addNode(ident, True) == 0
    shift = lom.Pose3D((0.05, -0.03, 0.0), (1, 0, 0, 0))
    for k, scan in enumerate((case["scan"], lom.transform_points(shift.inverse(), case["scan"]))):
        pose = matcher.align(grid, scan, lom.Pose3D())
        rep = lom.quality_report(grid, scan, pose, raw=True)
        z = np.concatenate([pose.translation, pose.rotation]).astype(np.float64)
        z[3:] /= np.linalg.norm(z[3:])
        assert pg.addNode(z, False) == k + 1
        assert pg.addEdge(0, k + 1, z, rep, 0.0) == k
    chi2 = pg.chi2()
    print("chi2 at the aligned poses:", chi2)
    om = lom.graph_information_from_quality(rep, True)
    assert np.all(chi2 <= 1e-24 * np.abs(om).max() * 36)  # e is zero to f64 rounding (1e-12 squared), weighed by Omega
    before = pg.poses()
    st = pg.optimize(gc.PARAMS)
    dt, dr = ref.pose_delta(pg.poses(), before)
    assert st["stop_reason"] == lom.capi.GRAPH_STOP_GRADIENT and dt < 1e-9 and dr < 1e-7
