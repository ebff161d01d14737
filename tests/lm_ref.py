"""Independent reference of the Levenberg-Marquardt policy of one ceres::Solve call of CloudMatcher::align.

Written from the semantics of Ceres 2.2 -- TrustRegionMinimizer (IterationZero, the main loop with
ParameterToleranceReached / FunctionToleranceReached before the step is judged, HandleSuccessfulStep /
HandleUnsuccessfulStep / HandleInvalidStep, GradientToleranceReached), LevenbergMarquardtStrategy (ComputeStep with the
clamped diagonal D of the scaled J^T J over the radius, StepAccepted / StepRejected / StepIsInvalid) and
QuaternionManifold::Plus -- with the options of the reference (max_num_iterations 4, function_tolerance 1e-5, defaults
otherwise), restated on the reduced 6x6 normal equations the product works with.

How independent it is: the NUMBERS are -- the linear solve, the definiteness test (eigenvalues, not pivots) and the
manifold step are done at 50 digits by other algorithms than the product's.  The POLICY part is a restatement of the same
Ceres functions that csrc/lm_core.hpp and oracle/oracle.c restate, in the same order of statements, because that order is
Ceres': a misreading of Ceres shared by all three would not show here; only the reference's own test vectors (through the
oracle) guard against that.

What makes it a reference and not a third implementation: the linear step comes from a 50-digit solve of
(S A S + D / radius) y = S g and the manifold step from 50-digit sin / cos, both rounded once to f64; the decisions are
then taken in f64 from those values, and every threshold comparison reports its relative margin, so that a test can
refuse cases in which rounding could legitimately flip a decision.  Non-finite inputs follow C fmax / fmin
(numpy.fmax / numpy.fmin): a NaN operand is ignored.

`evaluations` counts evaluated POINTS (iteration 0 and every candidate), which is what the product counts; Ceres
evaluates an accepted candidate a second time for its Jacobian.
"""
import numpy as np
from mpmath import mp, mpf

LM_DONE, LM_EVAL = 0, 1
MAX_ITER = 4
FTOL, GTOL, PTOL = 1e-5, 1e-10, 1e-8
MIN_REL_DEC, MIN_DIAG, MAX_DIAG, MAX_RADIUS = 1e-3, 1e-6, 1e32, 1e16
PRIOR_W = 10.0   # NormalPrior with sqrt information diag(0.1)^-1 on the translation
EPS = float(np.finfo(np.float64).eps)
DPS = 50


def assemble(sums, x, prior_b):
    """32-double block (prior excluded) -> A (6x6), g (6), cost with the NormalPrior residual 10 (t - b) added."""
    s = np.asarray(sums, np.float64)
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = s[k]
            k += 1
    g = s[21:27].copy()
    cost = np.float64(s[27])
    r = PRIOR_W * (np.asarray(x, np.float64)[4:7] - np.asarray(prior_b, np.float64))
    for a in range(3):
        A[3 + a, 3 + a] += PRIOR_W * PRIOR_W
        g[3 + a] += PRIOR_W * r[a]
        cost = cost + 0.5 * r[a] * r[a]
    return A, g, cost


def _margin(a, b):
    """relative distance of the two sides of a comparison; None when either is not finite (an exact case)"""
    if not (np.isfinite(a) and np.isfinite(b)):
        return None
    m = max(abs(a), abs(b))
    return 1.0 if m == 0.0 else abs(a - b) / m


def _gmax(g):
    m = np.float64(0.0)
    for v in g:
        m = np.fmax(m, abs(v))
    return m


def _plus(x, delta):
    """QuaternionManifold::Plus on [w x y z] (q_delta = [cos|d|, sin|d| / |d| d] applied on the left), translation
    added; 50 digits, rounded once."""
    d = [mpf(float(v)) for v in delta]
    xq = [mpf(float(v)) for v in x[:4]]
    n = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if n == 0:
        q = xq
    else:
        s = mp.sin(n) / n
        z = [mp.cos(n), s * d[0], s * d[1], s * d[2]]
        q = [z[0] * xq[0] - z[1] * xq[1] - z[2] * xq[2] - z[3] * xq[3],
             z[0] * xq[1] + z[1] * xq[0] + z[2] * xq[3] - z[3] * xq[2],
             z[0] * xq[2] - z[1] * xq[3] + z[2] * xq[0] + z[3] * xq[1],
             z[0] * xq[3] + z[1] * xq[2] - z[2] * xq[1] + z[3] * xq[0]]
    t = [mpf(float(x[4 + i])) + d[3 + i] for i in range(3)]
    return np.array([float(v) for v in q + t], np.float64), float(n)


def _solve50(M, b):
    """(y rounded to f64, cond2(M), lam_min / lam_max) of the symmetric M at 50 digits; y is None when M
    is not positive definite (the product's "non-positive pivot": the pivots of an elimination without row exchanges
    are all positive exactly for a positive definite matrix)."""
    Mm = mp.matrix(6, 6)
    for a in range(6):
        for c in range(6):
            Mm[a, c] = mpf(float(M[a, c]))
    ev = mp.eigsy(Mm, eigvals_only=True)
    lo, hi = min(ev), max(ev)
    rel = float(lo / max(abs(lo), abs(hi))) if (lo != 0 or hi != 0) else 0.0
    if not lo > 0:
        return None, 0.0, rel
    y = mp.lu_solve(Mm, mp.matrix([mpf(float(v)) for v in b]))
    return np.array([float(v) for v in y], np.float64), float(hi / lo), rel


def solve(x0, prior_b, sums_at):
    """Runs the policy from x0; `sums_at(x)` -> the 32-double block at x.  Returns one dict per evaluation:
    action, point (the candidate, or the solution when done), events (set of branch tags), tag (the events joined),
    recorded, evaluations, last_step_norm, cost (running), x (the point evaluated), sums, margins [(name, margin)],
    and for a proposed step: y, scale, cond, half_angle, bound (see point_bound)."""
    with mp.workdps(DPS):
        return _solve(np.asarray(x0, np.float64), np.asarray(prior_b, np.float64), sums_at)


def _solve(x, prior_b, sums_at):
    out = []
    st = dict(recorded=1, evaluations=1, last_step_norm=0.0)
    sums = np.asarray(sums_at(x), np.float64)
    A, g, cost = assemble(sums, x, prior_b)
    with np.errstate(all="ignore"):
        scale = 1.0 / (1.0 + np.sqrt(np.diag(A)))
    x_norm = np.sqrt(np.sum(x * x))
    radius, dec, reuse_diag, invalid_run = np.float64(1e4), np.float64(2.0), False, 0
    diag = np.zeros(6)
    it = 1
    ev = dict(x=x.copy(), sums=sums, events=["begin"], margins=[])
    if np.any(np.diag(A) == 0.0):
        ev["events"].append("zero_row")

    def close(action, point, extra=None):
        ev.update(action=action, point=np.asarray(point, np.float64).copy(), cost=float(cost), **st)
        ev.update(extra or {})
        ev["tag"] = "+".join(ev["events"])
        out.append(dict(ev))

    gm = _gmax(g)
    ev["margins"].append(("gtol", _margin(gm, GTOL)))
    if gm <= GTOL:
        ev["events"].append("gtol0")
        close(LM_DONE, x)
        return out
    while True:
        # ---- propose: steps until one is worth an evaluation, or the iteration budget is spent
        proposal = None
        while it <= MAX_ITER:
            with np.errstate(all="ignore"):
                As = A * scale[:, None] * scale[None, :]
                gs = g * scale
                if not reuse_diag:
                    raw = np.diag(As).copy()
                    diag = np.fmin(np.fmax(raw, MIN_DIAG), MAX_DIAG)
                    if np.any(raw < MIN_DIAG):
                        ev["events"].append("clamp")
                else:
                    ev["events"].append("reuse_diag")
                M = As + np.diag(diag / radius)
            reuse_diag = True
            valid = bool(np.all(np.isfinite(M)) and np.all(np.isfinite(gs)))
            if valid:
                y, cond, lam_rel = _solve50(M, gs)
                valid = y is not None
                # the sign of the smallest eigenvalue decides where it is negative, and in the first positive definite
                # solve after such steps; a sum of w J J^T plus a positive diagonal is never near that edge
                if not valid or invalid_run:
                    ev["margins"].append(("positive_definite", min(1.0, abs(lam_rel))))
            if valid:
                step = -y
                gsdot = float(np.dot(gs, step))
                quad = float(step @ As @ step)
                model_change = -gsdot - 0.5 * quad
                ev["margins"].append(("model_change", _margin(-gsdot, 0.5 * quad)))
                valid = bool(np.all(np.isfinite(y))) and model_change > 0.0
            if not valid:
                ev["events"].append("invalid")
                invalid_run += 1
                if invalid_run >= 5:
                    break
                radius = radius / dec
                dec = dec * 2.0
                st["recorded"] += 1
                st["last_step_norm"] = 0.0
                it += 1
                continue
            if invalid_run:
                ev["events"].append("valid_after_invalid")
            invalid_run = 0
            delta = step * scale
            cand, half_angle = _plus(x, delta)
            if delta[0] == 0.0 and delta[1] == 0.0 and delta[2] == 0.0:
                ev["events"].append("n2zero")
            else:
                ev["events"].append("ha_lo" if half_angle < 0.05 else ("ha_mid" if half_angle < 0.5 else "ha_hi"))
                if 0.45 <= half_angle < 0.5 and cond < 10.0:
                    ev["events"].append("ha_mid_top")      # where a series meant for < 0.05 is wrong beyond the bound
            if cond > 1e8:
                ev["events"].append("illcond")
            proposal = dict(y=y, scale=scale.copy(), cond=cond, half_angle=half_angle)
            proposal["bound"] = point_bound(proposal, x)
            break
        if proposal is None:
            ev["events"].append("budget" if it > MAX_ITER else "invalid_budget")
            close(LM_DONE, x)
            return out
        ev["events"].append("eval")
        close(LM_EVAL, cand, proposal)
        # ---- feed: the evaluation at the candidate
        sums = np.asarray(sums_at(cand), np.float64)
        ev = dict(x=cand.copy(), sums=sums, events=[], margins=[])
        st["evaluations"] += 1
        C_A, C_g, C_cost = assemble(sums, cand, prior_b)
        sn = np.sqrt(np.sum((x - cand) ** 2))
        ev["margins"].append(("ptol", _margin(sn, PTOL * (x_norm + PTOL))))
        if sn <= PTOL * (x_norm + PTOL):
            ev["events"].append("ptol")
            close(LM_DONE, x)
            return out
        with np.errstate(all="ignore"):
            cost_change = cost - C_cost
            ev["margins"].append(("ftol", _margin(abs(cost_change), FTOL * cost)))
            if abs(cost_change) <= FTOL * cost:
                ev["events"].append("ftol")
                close(LM_DONE, x)
                return out
            rel_dec = cost_change / model_change
            ev["margins"].append(("rel_dec", _margin(rel_dec, MIN_REL_DEC)))
            if rel_dec > MIN_REL_DEC:
                ev["events"].append("accept")
                x, A, g, cost = cand, C_A, C_g, C_cost
                x_norm = np.sqrt(np.sum(x * x))
                d3 = 2.0 * rel_dec - 1.0
                radius = np.fmin(MAX_RADIUS, radius / np.fmax(1.0 / 3.0, 1.0 - d3 * d3 * d3))
                dec = np.float64(2.0)
                reuse_diag = False
            else:
                ev["events"].append("reject_again" if out[-1]["events"][0] in ("reject", "reject_again") else "reject")
                radius = radius / dec
                dec = dec * 2.0
                reuse_diag = True
        st["recorded"] += 1
        st["last_step_norm"] = float(sn)
        gm = _gmax(g)
        ev["margins"].append(("gtol", _margin(gm, GTOL)))
        if gm <= GTOL:
            ev["events"].append("gtol")
            close(LM_DONE, x)
            return out
        it += 1


def point_bound(p, x):
    """Bound, per component of the 7-vector, of |proposed point - this reference's| for an implementation that solves
    the 6x6 system in f64 by elimination with 2-ulp reciprocals.

    Tangent component c of the step: 64 eps cond2(M) max|y| scale_c (6 elimination steps with their growth plus the
    reciprocals, rounded up to a power of two), cond2 and y from the 50-digit solve.  A translation component takes its
    tangent component's bound; a quaternion component the largest of the three rotation components' (|q| is 1 to
    rounding and q_delta * q mixes the three).  8 eps |x|_2 is added for the quaternion product and the series.
    Nothing is added for the distance between a replayed policy's own previous point and this reference's."""
    y, scale, cond = p["y"], p["scale"], p["cond"]
    tb = 64.0 * EPS * cond * float(np.max(np.abs(y))) * scale
    b = np.empty(7)
    b[:4] = float(np.max(tb[:3]))
    b[4:] = tb[3:]
    return b + 8.0 * EPS * float(np.sqrt(np.sum(np.asarray(x, np.float64) ** 2)))


def min_margin(trace):
    """the thinnest finite margin over every comparison of a solve (1.0 when there is none)"""
    m = [v for e in trace for _, v in e["margins"] if v is not None]
    return min(m) if m else 1.0
