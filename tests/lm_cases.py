"""Small problems for the LM policy tests: the policy sees only the 32 sums of an evaluation, so a problem is a handful
of (source point, map point, normal) correspondences evaluated in f64 numpy.

`eval_sums` restates PointToPlaneErrorAnalytic::Evaluate (reference src/cloud_matcher.cpp:38-103: residual
n . (q * p + t - o), the four dR/dq_i matrices), ceres::HuberLoss(0.15) (:134) and Ceres' QuaternionManifold
plus-Jacobian (:121) into the block layout of lom_debug_eval_sums (21 upper-triangle entries of sum w J J^T, sum w J r
at 21..26, sum 0.5 rho at 27, counters, the NormalPrior NOT included: lm_assemble adds it).  It is pinned against
oracle.Shard.eval_fixed by tests/test_lm_policy_host.py.

`all_cases()` builds every case once (deterministic seeds), runs the reference (tests/lm_ref.py) on it and records the
sequence (x_e, sums_e) the REFERENCE visits: the replay hands a policy under test the sums taken at those points.

What the point bound (lm_ref.point_bound, the formula 64 eps cond2(M) max|y| scale_c) does NOT constrain: in the
zero-normal and single-plane cases (prior_only_far_*, zero_normals_off_prior_*, one_plane_*, and the invalid-step cases'
kin) cond2(M) is 1e10 to 2e11 only because of the clamped 1e-6 / radius on the diagonal of a block-diagonal matrix; the
bound comes out at metres and more, so for the clamp, zero-row and gtol-after-accept branches only the decisions,
last_step_norm and cost are checked in earnest.  Those cases also carry most of the `illcond` tags; the coupled
ill-conditioned systems are near_origin_* (cond2 1.2e8 to 2.1e8, a near-null direction that is no coordinate axis).
near_parallel_* reaches 2e4 to 2e5 only: with the prior's 100 on the translation diagonal and D / radius >= 1e-4 of a
scaled diagonal near 1, two nearly parallel plane families cannot go higher.
"""
import functools

import numpy as np

from tests import lm_ref

HUBER_A = 0.15
MARGIN = 1e-6     # a case is admitted only if every threshold comparison of the reference is at least this far from flipping


def quat_from_rotvec(v):
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a == 0.0:
        return np.array([1.0, 0, 0, 0])
    return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * v / a])


def quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def rotate(q, p):
    """q * p the way Eigen evaluates it (q need not be a unit quaternion): p + w 2(u x p) + u x 2(u x p)"""
    u = np.asarray(q[1:4], np.float64)
    t2 = 2.0 * np.cross(np.broadcast_to(u, p.shape), p)
    return p + q[0] * t2 + np.cross(np.broadcast_to(u, p.shape), t2)


def eval_sums(P, O, N, x):
    """the 32-double block at x = [qw qx qy qz tx ty tz] for the correspondences (P[i], O[i], N[i])"""
    x = np.asarray(x, np.float64)
    w, a, b, c = x[:4]
    out = np.zeros(32)
    n = len(P)
    out[28] = out[31] = n
    if n == 0:
        return out
    r = np.sum((rotate(x[:4], P) + x[4:7] - O) * N, axis=1)
    dR = 2.0 * np.array([[[w, -c, b], [c, w, -a], [-b, a, w]],
                         [[a, b, c], [b, -a, -w], [c, w, -a]],
                         [[-b, a, w], [a, b, c], [-w, c, -b]],
                         [[-c, -w, a], [w, -c, b], [a, b, c]]])
    ja = np.einsum("kij,nj,ni->nk", dR, P, N)                       # d r / d q_k
    plus = np.array([[-a, -b, -c], [w, c, -b], [-c, w, a], [b, -a, w]])
    J = np.concatenate([ja @ plus, N], axis=1)                      # tangent row: rotation(3), translation(3)
    s = r * r
    knee = HUBER_A * HUBER_A
    big = s > knee
    root = np.sqrt(np.where(big, s, 1.0))
    rho0 = np.where(big, 2.0 * HUBER_A * root - knee, s)
    rho1 = np.where(big, np.maximum(HUBER_A / root, np.finfo(np.float64).tiny), 1.0)
    A = np.einsum("n,ni,nj->ij", rho1, J, J)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            out[k] = A[i, j]
            k += 1
    out[21:27] = np.einsum("n,ni,n->i", rho1, J, r)
    out[27] = 0.5 * np.sum(rho0)
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------
def planes(rng, normals, n_each, half=3.0, centre=(0, 0, 0), offset=2.0):
    """map points on one plane per normal, `offset` from `centre` along the normal; (O, N)"""
    O, N = [], []
    for nrm in normals:
        nrm = np.asarray(nrm, np.float64)
        nrm = nrm / np.linalg.norm(nrm)
        e1 = np.cross(nrm, [0.3, -0.5, 0.8])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(nrm, e1)
        uv = rng.uniform(-half, half, (n_each, 2))
        O.append(np.asarray(centre, np.float64) + offset * nrm + uv[:, :1] * e1 + uv[:, 1:] * e2)
        N.append(np.tile(nrm, (n_each, 1)))
    return np.concatenate(O), np.concatenate(N)


def source_of(O, N, q_true, t_true, along=None):
    """source points that land on their map points at the true pose (plus `along` metres along the normal)"""
    qi = np.array([q_true[0], -q_true[1], -q_true[2], -q_true[3]])
    W = O if along is None else O + np.asarray(along, np.float64)[:, None] * N
    return rotate(qi, W - np.asarray(t_true, np.float64))


BOX = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


def _case(name, recipe, P, O, N, x0, prior_b, corrupt=None):
    return dict(name=name, recipe=recipe, P=np.asarray(P, np.float64), O=np.asarray(O, np.float64),
                N=np.asarray(N, np.float64), x0=np.asarray(x0, np.float64), prior_b=np.asarray(prior_b, np.float64),
                corrupt=corrupt)


def _guess(rotvec, dt, t_true=(0, 0, 0)):
    return np.concatenate([quat_from_rotvec(rotvec), np.asarray(t_true, np.float64) + np.asarray(dt, np.float64)])


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def generate():
    """every generated case, admitted or not"""
    cases = []
    # accepted steps only: a box corner, the guess 2 cm / 0.01 rad off
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        O, N = planes(rng, BOX, 12)
        P = source_of(O, N, (1, 0, 0, 0), (0, 0, 0))
        x0 = _guess(0.01 * _unit(rng), 0.02 * _unit(rng))
        cases.append(_case(f"box_near_{seed}", "accepted", P, O, N, x0, x0[4:]))
    # rejected steps: few points far from the origin, residuals on both sides of the Huber knee, the guess far off
    # (seeds and angles picked, with the reference alone, for the order of rejected and accepted steps they give)
    for seed, ang in ((104, 0.9), (112, 0.5), (105, 0.7), (100, 1.0), (104, 1.2), (111, 1.2)):
        rng = np.random.default_rng(seed)
        centre = _unit(rng) * rng.uniform(30, 80)
        O, N = planes(rng, BOX, 2 + seed % 2, half=4.0, centre=centre)
        P = source_of(O, N, (1, 0, 0, 0), (0, 0, 0), along=rng.choice([0.0, 0.05, 0.3, -0.4], len(O)))
        x0 = _guess(ang * _unit(rng), 0.1 * _unit(rng))
        cases.append(_case(f"far_{seed}_{ang}", "rejected", P, O, N, x0, x0[4:]))
    # gradient tolerance at iteration 0: every point on its plane and t == prior_b (g exactly 0); zero normals
    for seed in (21, 22):
        rng = np.random.default_rng(seed)
        O, N = planes(rng, BOX, 5)
        x0 = np.array([1.0, 0, 0, 0, 0, 0, 0])
        cases.append(_case(f"on_planes_{seed}", "gtol0", O.copy(), O, N, x0, x0[4:]))
        t = rng.uniform(-5, 5, 3)
        x0 = _guess(0.2 * _unit(rng), (0, 0, 0), t)
        cases.append(_case(f"zero_normals_at_prior_{seed}", "gtol0", O + 0.1, O, np.zeros_like(N), x0, x0[4:]))
    # gradient tolerance after an accepted step: zero normals leave the prior alone, a LINEAR problem in t whose
    # damped Gauss-Newton steps shrink t - b by 1 / radius each (radius 1e4, 3e4, 9e4, 2.7e5): from 2e6 m the fourth
    # step is longer than the parameter tolerance and lands on |g| = 100 |t - b| < 1e-10.  (The recipe of a plane
    # problem inside the knee cannot do it: with the prior's 100 on the diagonal a step that reaches g <= 1e-10 is
    # shorter than 1e-8 |x|, and the parameter tolerance stops the solve first.)  The block carries a constant cost of
    # 1e-8, small enough for the function tolerance to stay out of the way: without it the final cost would be
    # 50 |t - b|^2 of the policy's OWN last point alone, a difference of rounded values that no two implementations share
    # to 1e-12.
    for seed, t0 in ((31, (2e6, 0, 0)), (32, (-1.5e6, 1.0e6, 0.5e6))):
        rng = np.random.default_rng(seed)
        O, N = planes(rng, BOX, 3)
        x0 = np.concatenate([quat_from_rotvec(0.1 * _unit(rng)), np.asarray(t0, np.float64)])
        def floor_cost(s):
            s[27] = 1e-8
        cases.append(_case(f"prior_only_far_{seed}", "gtol_after_accept", O + 0.2, O, np.zeros_like(N), x0, np.zeros(3),
                           corrupt=floor_cost))
    # parameter tolerance: the guess 1e-10 off the optimum
    for seed in (41, 42):
        rng = np.random.default_rng(seed)
        O, N = planes(rng, BOX, 6)
        x0 = np.array([1.0, 0, 0, 0, 0, 0, 0])
        x0[4:] += 1e-10 * _unit(rng)
        cases.append(_case(f"at_optimum_{seed}", "ptol", O.copy(), O, N, x0, np.zeros(3)))
    # function tolerance: outliers beyond the knee carry a large constant cost, the guess 1e-4 off
    for seed in (51, 52):
        rng = np.random.default_rng(seed)
        O, N = planes(rng, BOX, 10)
        along = np.where(np.arange(len(O)) % 2 == 0, 0.0, np.where(np.arange(len(O)) % 4 == 1, 1.0, -1.0))
        P = source_of(O, N, (1, 0, 0, 0), (0, 0, 0), along=along)
        x0 = _guess(1e-4 * _unit(rng), 1e-4 * _unit(rng))
        cases.append(_case(f"outliers_{seed}", "ftol", P, O, N, x0, x0[4:]))
    # zero rows / minimum diagonal: one plane family only; zero normals with the guess off the prior
    for seed in (61, 62):
        rng = np.random.default_rng(seed)
        O, N = planes(rng, ((0, 0, 1),), 20)
        P = source_of(O, N, (1, 0, 0, 0), (0, 0, 0))
        x0 = _guess(0.02 * _unit(rng), 0.05 * _unit(rng))
        cases.append(_case(f"one_plane_{seed}", "clamp", P, O, N, x0, x0[4:]))
        O, N = planes(rng, BOX, 4)
        x0 = _guess(0.3 * _unit(rng), rng.uniform(-1, 1, 3))
        cases.append(_case(f"zero_normals_off_prior_{seed}", "zero_rows", O + 0.1, O, np.zeros_like(N), x0,
                           x0[4:] + rng.uniform(-0.5, 0.5, 3)))
    # ill-conditioned: two plane families 1e-4 rad apart; points within 1 mm of the rotation axis
    for seed in (71, 72):
        rng = np.random.default_rng(seed)
        n1 = _unit(rng)
        n2 = n1 + 1e-4 * np.cross(n1, _unit(rng))
        O, N = planes(rng, (n1, n2), 32, half=20.0)
        P = source_of(O, N, (1, 0, 0, 0), (0, 0, 0), along=rng.uniform(-0.05, 0.05, len(O)))
        x0 = _guess(0.01 * _unit(rng), 0.03 * _unit(rng))
        cases.append(_case(f"near_parallel_{seed}", "illcond", P, O, N, x0, x0[4:]))
        # a cluster 1 mm from the origin: every rotation is weakly seen (small scaled diagonal, so D / radius is tiny)
        # and the rotation about the cluster's direction hardly at all -- a near-null direction that is no coordinate axis
        p0 = 1e-3 * _unit(rng)
        W = p0 + 1e-5 * rng.uniform(-1, 1, (48, 3))
        N = np.array([_unit(rng) for _ in range(48)])
        P = W.copy()
        O = W - rng.uniform(-1e-5, 1e-5, 48)[:, None] * N
        x0 = _guess(0.01 * _unit(rng), 2e-5 * _unit(rng))
        cases.append(_case(f"near_origin_{seed}", "illcond", P, O, N, x0, x0[4:]))
    # the step's half-angle: a well-constrained box, the guess 0.4 rad and 1.3 rad off
    for seed, ang in ((81, 0.4), (82, 0.4), (83, 1.3), (84, 1.3)):
        rng = np.random.default_rng(seed)
        O, N = planes(rng, BOX + ((-1, 0, 0), (0, -1, 0), (0, 0, -1)), 8, half=2.0, offset=0.5)
        P = source_of(O, N, (1, 0, 0, 0), (0, 0, 0))
        x0 = _guess(ang * _unit(rng), 0.01 * _unit(rng))
        cases.append(_case(f"box_turned_{ang}_{seed}", "half_angle", P, O, N, x0, x0[4:]))
    # the top of the middle range: a box of 0.16 m (every residual inside the knee, so the first Gauss-Newton step takes
    # most of the 1.2 rad) gives a first half-angle of 0.49 at cond2 7 to 8.  The cosine series cut after z^5 / 10! would
    # be wrong by 0.49^12 / 12! = 4e-13 there, against a bound of 5e-14: what tells a < 0.05 from a < 0.5 in
    # lmw2_sinc_cos.  (Seeds picked with the reference alone for that half-angle.)
    for seed in (304, 305, 311):
        rng = np.random.default_rng(seed)
        O, N = planes(rng, BOX + ((-1, 0, 0), (0, -1, 0), (0, 0, -1)), 10, half=0.08, offset=0.05)
        P = source_of(O, N, (1, 0, 0, 0), (0, 0, 0))
        x0 = _guess(1.2 * _unit(rng), 0.001 * _unit(rng))
        cases.append(_case(f"small_box_turned_{seed}", "half_angle", P, O, N, x0, x0[4:]))
    rng = np.random.default_rng(91)
    O, N = planes(rng, BOX, 8)
    P = source_of(O, N, (1, 0, 0, 0), (0, 0, 0))
    x0 = _guess(0.01 * _unit(rng), 0.02 * _unit(rng))
    # invalid steps with finite sums: zero normals leave the prior's diag(100, 100, 100) on the translation; with a
    # rotation block set to I, A[3][4] = 100 (1 + e) makes the system indefinite until the damping 1 + 1 / radius exceeds
    # 1 + e.  The radius goes 1e4, 5e3, 1250, 156.
    Oz, Nz = planes(rng, BOX, 3)
    xz = _guess(0.1 * _unit(rng), (3e-5, -2e-5, 1e-5))
    for name, e in (("two_invalid", 5e-4), ("three_invalid", 3e-3)):
        def push(s, e=e):
            s[0] = s[6] = s[11] = 1.0
            s[16] = 100.0 * (1.0 + e)
        cases.append(_case(f"indefinite_{name}", "invalid_then_valid", Oz + 0.1, Oz, np.zeros_like(Nz), xz, np.zeros(3),
                           corrupt=push))
    # non-finite sums: every step is invalid, the iteration budget ends the solve.  (A NaN COST does not enter the linear
    # system: its steps are valid and each candidate is rejected, rel_dec being NaN -- four rejections, same exit.)
    for name, idx, val in (("A_diag_inf", 0, np.inf), ("A_offdiag_inf", 8, np.inf), ("A_nan", 3, np.nan),
                           ("g_nan", 23, np.nan), ("cost_nan", 27, np.nan)):
        def put(s, idx=idx, val=val):
            s[idx] = val
        cases.append(_case(f"nonfinite_{name}", "nonfinite", P, O, N, x0, x0[4:], corrupt=put))
    return cases


def sums_fn(case):
    def f(x):
        s = eval_sums(case["P"], case["O"], case["N"], x)
        if case["corrupt"] is not None:
            case["corrupt"](s)
        return s
    return f


@functools.lru_cache(maxsize=None)
def all_cases():
    """(admitted, dropped): every case with its reference trace under "trace"; computed once per process"""
    admitted, dropped = [], []
    for c in generate():
        c["trace"] = lm_ref.solve(c["x0"], c["prior_b"], sums_fn(c))
        assert len(c["trace"]) <= 5
        (admitted if lm_ref.min_margin(c["trace"]) >= MARGIN else dropped).append(c)
    return tuple(admitted), tuple(dropped)


def as_solve(case):
    """the argument of lom.debug_lm_policy for a case: the sums at the reference's points"""
    return case["x0"], case["prior_b"], np.array([e["sums"] for e in case["trace"]])


def check_solve(case, got, what):
    """One policy form's replay of a case (a dict of lom.debug_lm_policy) against the reference trace.  Returns the worst
    ratio of a proposed point's error to its derived bound (0.0 when nothing was proposed)."""
    tr = case["trace"]
    name = (what, case["name"])
    assert got["actions"] == [e["action"] for e in tr], (name, got["actions"], [e["tag"] for e in tr])
    assert got["recorded"] == tr[-1]["recorded"], (name, got["recorded"], tr[-1]["recorded"])
    assert got["evaluations"] == tr[-1]["evaluations"], (name, got["evaluations"], tr[-1]["evaluations"])
    if case["recipe"] == "nonfinite":
        return 0.0
    assert abs(got["last_step_norm"] - tr[-1]["last_step_norm"]) <= 1e-13, (name, got["last_step_norm"], tr[-1]["last_step_norm"])
    assert abs(got["cost"] - tr[-1]["cost"]) <= 1e-12 * abs(tr[-1]["cost"]), (name, got["cost"], tr[-1]["cost"])
    worst = 0.0
    # a finished solve's solution is the last ACCEPTED candidate, the policy's own: that proposal's bound holds for it
    accepted = np.zeros(7)
    last = None
    for e, pt in zip(tr, got["points"]):
        if e["events"][0] == "accept":
            accepted = last
        if e["action"] == lm_ref.LM_EVAL:
            bound = last = e["bound"]
        else:
            bound = accepted + 8.0 * lm_ref.EPS * np.sqrt(np.sum(e["point"] ** 2))
        err = np.abs(pt - e["point"])
        assert np.all(err <= bound), (name, e["tag"], err, bound)
        if e["action"] == lm_ref.LM_EVAL:
            worst = max(worst, float(np.max(err / bound)))
    return worst
