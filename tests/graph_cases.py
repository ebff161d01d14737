"""The graphs the pose-graph tests share (tests/graph_ref.py builds them), the solver parameters, and the reference's
optimum of each, computed once per process."""
import functools

import numpy as np

from tests import graph_ref as ref

# gtol.  Two floors lie below it.  (1) The rounding floor of g itself, about 1e-16 * g_abs ~ 1e-7 on these graphs.  (2) The
# gain test of the contract accepts a step only if cost - cost_new > 0, and that difference of two sums of m terms carries
# rounding noise of about 1.1e-16 * cost * sqrt(m) (cost up to 1.4e3, m up to 1e3: some 1e-12), while the decrease a step
# can still win is about g^2 / (2 h) with h, the curvature, 1e4 to 2e6 here: below |g| of about 1e-4 the sign of the gain
# is noise, every step is refused, lambda grows and the solver ends on xtol -- the reference and the device alike, each
# with its own rounding.  1e-3 stays a decade above that; with h >= 2.5e3 it pins the poses to 4e-7, far inside the 1e-4
# pose-parity bar.
PARAMS = dict(lambda0=1e-4, gtol=1e-3, xtol=1e-12, pcg_rtol=1e-8, max_outer=30, max_pcg=200)
POSE_BAR = 1e-4  # m and rad: the project's pose-parity bar

CASES = ("n2", "n7_duplicates", "n65", "n65_two_fixed", "n257", "n600_hubs")


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, truth); the arrays are shared: copy before changing one"""
    if name == "n1":
        return ref.ring_with_spokes(1, 1)
    if name == "n2":
        return ref.ring_with_spokes(2, 2)
    if name == "n7_duplicates":
        g, truth = ref.ring_with_spokes(7, 7)
        dup = [0, 3, 3, 8]  # edges 0, 3 (twice) and 8 once more, with the same measurement and another Omega
        rng = np.random.default_rng(77)
        g = dict(g, ij=np.concatenate([g["ij"], g["ij"][dup]]), Z=np.concatenate([g["Z"], g["Z"][dup]]),
                 Om=np.concatenate([g["Om"], ref.random_spd(rng, len(dup))]), delta=np.concatenate([g["delta"], g["delta"][dup]]))
        return g, truth
    if name == "n65":
        return ref.ring_with_spokes(65, 65)
    if name == "n65_two_fixed":
        g, truth = ref.ring_with_spokes(65, 66)
        fixed = g["fixed"].copy()
        fixed[32] = True
        poses = g["poses"].copy()
        poses[32] = truth[32]
        return dict(g, fixed=fixed, poses=poses), truth
    if name == "n257":
        return ref.ring_with_spokes(257, 257)
    if name == "n600_hubs":
        return ref.ring_with_spokes(600, 600, second_hub=True)
    if name == "n65_exact":
        return ref.ring_with_spokes(65, 67, noise=False)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def optimum(name, count_pcg=False):
    """(poses, stats) of graph_ref.lm on the case"""
    return ref.lm(case(name)[0], PARAMS, count_pcg=count_pcg)


def with_huber(graph, poses, share=1.0 / 3.0):
    """the graph with one delta for all edges that puts `share` of them on the Huber branch at `poses`; delta^2 lies
    midway between two neighbouring s, so that no edge sits on the branch point"""
    s = np.sort(ref.linearise(dict(graph, delta=np.zeros(len(graph["ij"]))), poses)["s"])
    k = int(round(len(s) * (1.0 - share)))
    delta = float(np.sqrt(0.5 * (s[k - 1] + s[k])))
    return dict(graph, delta=np.full(len(s), delta))


def build(lom, graph, poses=None, bulk=True, hints=(0, 0)):
    """a lom.PoseGraph holding the graph (at `poses` if given)"""
    pg = lom.PoseGraph(*hints)
    poses = graph["poses"] if poses is None else poses
    if bulk:
        pg.addNodes(poses, graph["fixed"])
        if len(graph["ij"]):
            pg.addEdges(graph["ij"], graph["Z"], graph["Om"], graph["delta"])
    else:
        for k in range(len(poses)):
            assert pg.addNode(poses[k], graph["fixed"][k]) == k
        for k in range(len(graph["ij"])):
            assert pg.addEdge(graph["ij"][k, 0], graph["ij"][k, 1], graph["Z"][k], graph["Om"][k], graph["delta"][k]) == k
    return pg
