"""numpy f64 reference of the pose graph, written from the contract in include/lidar_odometry_amd.h ("pose graph") and not
from the device code: rotation matrices and a matrix logarithm where the device works on quaternions, one dense H where the
device has a CSR and whitened blocks, a dense Cholesky solve where it runs PCG.

A graph is a dict: poses (n, 7) [t, q wxyz], fixed (n,) bool, ij (m, 2), Z (m, 7), Om (m, 6, 6), delta (m,).

Sums of absolute terms.  The GPU tests hold every device value to REL times "the sum of the absolute values of its terms".
A value here is a sum of products of intermediates that are rounded sums themselves (e is made of R_i^T (t_j - t_i) with
coordinates of tens of metres, A holds t_ij), so the terms are taken down to the inputs: e_abs is e's own sum (the matrix
products with every factor replaced by its absolute value), A_abs is |A| plus the same for A's entries, and
    s_abs  = |e|^T |Om| |e| + 2 e_abs^T |Om| |e|          (first order in e's rounding)
    cost_abs = sum 0.5 w s_abs                            (d rho / ds = w <= 1)
    g_abs  = sum w A_abs^T |Om| (|e| + e_abs)
    H_abs  = sum w A_abs^T |Om| A_abs  (+ lambda on the diagonal)
    y_abs  = sum w A_abs^T |Om| (A_abs_i |p_i| + A_abs_j |p_j|) + lambda D |p|
"""
import numpy as np

REL = 1e-12  # tests/test_eval_parity.py holds the align's f64 sums to the same
STOP_GRADIENT, STOP_STEP, STOP_MAX_OUTER = 1, 2, 3


# ---- rotations ------------------------------------------------------------------------------------------------------
def quat_R(q):
    q = np.asarray(q, np.float64)
    w, x, y, z = np.moveaxis(q, -1, 0)
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z)
    R[..., 0, 1] = 2 * (x * y - w * z)
    R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z)
    R[..., 1, 1] = 1 - 2 * (x * x + z * z)
    R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y)
    R[..., 2, 1] = 2 * (y * z + w * x)
    R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def quat_mul(a, b):
    aw, ax, ay, az = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def quat_exp(a):
    """the unit quaternion of the rotation vector a"""
    a = np.asarray(a, np.float64)
    th = np.linalg.norm(a, axis=-1, keepdims=True)
    small = th < 1e-6
    k = np.where(small, 0.5 - th * th / 48.0, np.sin(0.5 * th) / np.where(small, 1.0, th))
    return np.concatenate([np.cos(0.5 * th), k * a], axis=-1)


def skew(v):
    v = np.asarray(v, np.float64)
    S = np.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -v[..., 2], v[..., 1]
    S[..., 1, 0], S[..., 1, 2] = v[..., 2], -v[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -v[..., 1], v[..., 0]
    return S


def so3_log(R):
    """rotation vector in (-pi, pi] of rotation matrices (angles up to about 3.1 rad: beyond, the antisymmetric part is
    too small to carry the axis)"""
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    s = np.linalg.norm(v, axis=-1)
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    th = np.arctan2(s, c)
    small = s < 1e-10
    k = np.where(small, 1.0 + s * s / 6.0, th / np.where(small, 1.0, s))
    return k[..., None] * v


def jl_inv(p):
    p = np.asarray(p, np.float64)
    th = np.linalg.norm(p, axis=-1)
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    c = np.where(small, 1.0 / 12.0, 1.0 / ths**2 - (1.0 + np.cos(ths)) / (2.0 * ths * np.sin(ths)))
    S = skew(p)
    return np.eye(3) - 0.5 * S + c[..., None, None] * (S @ S)


# ---- one edge (batched over the leading axis) ---------------------------------------------------------------------------
def error(Xi, Xj, Z, with_abs=False):
    """e = [ Log(R_i^T R_j R_z^T) ; R_i^T (t_j - t_i) - t_z ] for poses of shape (..., 7)"""
    Xi, Xj, Z = (np.asarray(a, np.float64) for a in (Xi, Xj, Z))
    Ri, Rj, Rz = quat_R(Xi[..., 3:]), quat_R(Xj[..., 3:]), quat_R(Z[..., 3:])
    RiT, RzT = np.swapaxes(Ri, -1, -2), np.swapaxes(Rz, -1, -2)
    E = RiT @ Rj @ RzT
    er = so3_log(E)
    tij = (RiT @ (Xj[..., :3] - Xi[..., :3])[..., None])[..., 0]
    e = np.concatenate([er, tij - Z[..., :3]], axis=-1)
    if not with_abs:
        return e
    absE = np.abs(RiT) @ np.abs(Rj) @ np.abs(RzT)
    th = np.linalg.norm(er, axis=-1)
    f = np.where(th < 1e-6, 0.5, th / (2.0 * np.sin(np.where(th < 1e-6, 1.0, th))))  # Log = f * (E - E^T)^vee
    er_abs = f[..., None] * np.stack([absE[..., 2, 1] + absE[..., 1, 2], absE[..., 0, 2] + absE[..., 2, 0],
                                      absE[..., 1, 0] + absE[..., 0, 1]], axis=-1)
    tij_abs = (np.abs(RiT) @ (np.abs(Xj[..., :3]) + np.abs(Xi[..., :3]))[..., None])[..., 0]
    return e, np.concatenate([er_abs, tij_abs + np.abs(Z[..., :3])], axis=-1), tij_abs


def jacobians(Xi, Xj, Z):
    """de/d(a_i, b_i), de/d(a_j, b_j), each (..., 6, 6)"""
    Xi, Xj, Z = (np.asarray(a, np.float64) for a in (Xi, Xj, Z))
    e = error(Xi, Xj, Z)
    Ri, Rz = quat_R(Xi[..., 3:]), quat_R(Z[..., 3:])
    RiT = np.swapaxes(Ri, -1, -2)
    tij = (RiT @ (Xj[..., :3] - Xi[..., :3])[..., None])[..., 0]
    Ai = np.zeros(e.shape[:-1] + (6, 6))
    Aj = np.zeros_like(Ai)
    Ai[..., :3, :3] = -jl_inv(e[..., :3])
    Ai[..., 3:, :3] = skew(tij)
    Ai[..., 3:, 3:] = -RiT
    Aj[..., :3, :3] = jl_inv(-e[..., :3]) @ Rz
    Aj[..., 3:, 3:] = RiT
    return Ai, Aj


def retract(poses, d, fixed):
    """R_k <- R_k Exp(a_k), t_k <- t_k + b_k for the free nodes; the quaternion re-normalised"""
    out = np.array(poses, np.float64)
    free = ~np.asarray(fixed, bool)
    q = quat_mul(out[free, 3:], quat_exp(d[free, :3]))
    out[free, 3:] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    out[free, :3] += d[free, 3:]
    return out


def huber(s, delta):
    """w, rho(s)"""
    plain = (delta == 0) | (s <= delta * delta)
    rs = np.sqrt(np.where(plain, 1.0, s))
    return np.where(plain, 1.0, delta / rs), np.where(plain, s, 2 * delta * rs - delta * delta)


def cost_of(graph, poses):
    ij = graph["ij"]
    if len(ij) == 0:
        return 0.0
    e = error(poses[ij[:, 0]], poses[ij[:, 1]], graph["Z"])
    s = np.einsum("ma,mab,mb->m", e, graph["Om"], e)
    return float(0.5 * huber(s, graph["delta"])[1].sum())


def linearise(graph, poses=None, lam=0.0):
    """dict: e, s, w (m ...), cost, g (n, 6), hdiag (n, 6, 6) = the diagonal blocks of H_ff + lam D, D (n, 6), the edge blocks
    Ai, Aj, and for every value its sum of absolute terms under `<name>_abs` (module docstring).  Fixed nodes read 0."""
    poses = graph["poses"] if poses is None else poses
    ij, Om, fixed = graph["ij"], graph["Om"], np.asarray(graph["fixed"], bool)
    n, m = len(poses), len(ij)
    Xi, Xj = poses[ij[:, 0]], poses[ij[:, 1]]
    e, e_abs, tij_abs = error(Xi, Xj, graph["Z"], with_abs=True)
    Ai, Aj = jacobians(Xi, Xj, graph["Z"])
    P = np.zeros((m, 6, 6))
    P[:, :3, :3] = 1.0
    P[:, 3:, 3:] = 1.0
    Pi = P.copy()
    Pi[:, 3:, :3] = np.abs(skew(tij_abs))
    Ai_abs, Aj_abs = np.abs(Ai) + Pi, np.abs(Aj) + P
    aOm, ae = np.abs(Om), np.abs(e)
    s = np.einsum("ma,mab,mb->m", e, Om, e)
    s_abs = np.einsum("ma,mab,mb->m", ae, aOm, ae) + 2 * np.einsum("ma,mab,mb->m", e_abs, aOm, ae)
    w, rho = huber(s, graph["delta"])
    out = {"e": e, "e_abs": e_abs, "s": s, "s_abs": s_abs, "w": w, "cost": float(0.5 * rho.sum()),
           "cost_abs": float(0.5 * (w * s_abs).sum()), "Ai": Ai, "Aj": Aj, "Ai_abs": Ai_abs, "Aj_abs": Aj_abs}
    g, g_abs = np.zeros((n, 6)), np.zeros((n, 6))
    H, H_abs = np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for side, (A, A_abs) in enumerate(((Ai, Ai_abs), (Aj, Aj_abs))):
        ge = w[:, None] * np.einsum("mka,mkl,ml->ma", A, Om, e)
        ge_abs = w[:, None] * np.einsum("mka,mkl,ml->ma", A_abs, aOm, ae + e_abs)
        He = w[:, None, None] * np.einsum("mka,mkl,mlb->mab", A, Om, A)
        He_abs = w[:, None, None] * np.einsum("mka,mkl,mlb->mab", A_abs, aOm, A_abs)
        for k in range(m):  # ascending edge id, as the contract has it
            nd = ij[k, side]
            g[nd] += ge[k]
            g_abs[nd] += ge_abs[k]
            H[nd] += He[k]
            H_abs[nd] += He_abs[k]
    D = np.einsum("naa->na", H).copy()
    idx = np.arange(6)
    H[:, idx, idx] += lam * D
    H_abs[:, idx, idx] += lam * np.einsum("naa->na", H_abs)
    for a in (g, g_abs, H, H_abs, D):
        a[fixed] = 0.0
    out.update(g=g, g_abs=g_abs, hdiag=H, hdiag_abs=H_abs, D=D)
    return out


def matvec(graph, lin, lam, p):
    """y = (H_ff + lam D) p and its sum of absolute terms; p (n, 6); a fixed node's p counts as 0 and its y reads 0"""
    ij, Om, fixed = graph["ij"], graph["Om"], np.asarray(graph["fixed"], bool)
    p = np.where(fixed[:, None], 0.0, np.asarray(p, np.float64))
    ap, aOm, w = np.abs(p), np.abs(Om), lin["w"]
    u = np.einsum("mab,mb->ma", lin["Ai"], p[ij[:, 0]]) + np.einsum("mab,mb->ma", lin["Aj"], p[ij[:, 1]])
    u_abs = np.einsum("mab,mb->ma", lin["Ai_abs"], ap[ij[:, 0]]) + np.einsum("mab,mb->ma", lin["Aj_abs"], ap[ij[:, 1]])
    y, y_abs = lam * lin["D"] * p, lam * lin["D"] * ap
    for side, (A, A_abs) in enumerate(((lin["Ai"], lin["Ai_abs"]), (lin["Aj"], lin["Aj_abs"]))):
        t = w[:, None] * np.einsum("mka,mkl,ml->ma", A, Om, u)
        t_abs = w[:, None] * np.einsum("mka,mkl,ml->ma", A_abs, aOm, u_abs)
        for k in range(len(ij)):
            y[ij[k, side]] += t[k]
            y_abs[ij[k, side]] += t_abs[k]
    y[fixed] = 0.0
    y_abs[fixed] = 0.0
    return y, y_abs


def dense_system(graph, lin):
    """H (6n x 6n) over all nodes and the list of free scalar indices"""
    n, ij, Om, w = len(graph["poses"]), graph["ij"], graph["Om"], lin["w"]
    H = np.zeros((6 * n, 6 * n))
    blocks = ((0, 0, lin["Ai"], lin["Ai"]), (0, 1, lin["Ai"], lin["Aj"]), (1, 0, lin["Aj"], lin["Ai"]),
              (1, 1, lin["Aj"], lin["Aj"]))
    for sa, sb, A, B in blocks:
        He = w[:, None, None] * np.einsum("mka,mkl,mlb->mab", A, Om, B)
        for k in range(len(ij)):
            a, b = ij[k, sa], ij[k, sb]
            H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += He[k]
    free = np.flatnonzero(np.repeat(~np.asarray(graph["fixed"], bool), 6))
    return H, free


def pcg(A, b, rtol, max_it):
    """block-Jacobi (6x6) preconditioned CG from x = 0 on the free system; returns x, iterations, capped"""
    nb = len(b) // 6
    Minv = np.stack([np.linalg.inv(A[6 * k:6 * k + 6, 6 * k:6 * k + 6]) for k in range(nb)]) if nb else np.zeros((0, 6, 6))
    prec = lambda r: np.einsum("kab,kb->ka", Minv, r.reshape(nb, 6)).reshape(-1)
    x, r = np.zeros_like(b), b.copy()
    z = prec(r)
    p, rz = z.copy(), float(r @ z)
    rz0 = rz
    if rz0 == 0.0:
        return x, 0, False
    for it in range(1, max_it + 1):
        y = A @ p
        alpha = rz / float(p @ y)
        x += alpha * p
        r -= alpha * y
        z = prec(r)
        rz_new = float(r @ z)
        if rz_new <= rtol * rtol * rz0:
            return x, it, False
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it, True


def lm_policy(cost, cost_new, denom, lam, nu):
    """one policy step: accepted, lambda, nu, rho_gain"""
    with np.errstate(all="ignore"):
        rho_gain = (np.float64(cost) - np.float64(cost_new)) / (np.float64(0.5) * np.float64(denom))
    if rho_gain > 0:
        t = 2.0 * rho_gain - 1.0
        return True, float(lam * max(1.0 / 3.0, 1.0 - t * t * t)), 2.0, float(rho_gain)
    return False, float(lam * nu), float(nu * 2.0), float(rho_gain)


def lm(graph, params, count_pcg=False):
    """Levenberg-Marquardt as the contract has it, the step by dense Cholesky.  Returns (poses, stats); with count_pcg the
    stats also hold the iterations the contract's PCG needs on every system solved (`pcg_iters`) and how many hit max_pcg."""
    poses = np.array(graph["poses"], np.float64)
    fixed = np.asarray(graph["fixed"], bool)
    n = len(poses)
    lam, nu = float(params["lambda0"]), 2.0
    st = {"outer": 0, "accepted": 0, "stop_reason": STOP_GRADIENT, "pcg_iters": [], "pcg_capped": 0, "cost_initial": 0.0,
          "cost_final": 0.0, "grad_max": 0.0, "lambda_final": lam}
    if len(graph["ij"]) == 0:
        return poses, st
    lin = linearise(graph, poses)
    st["cost_initial"] = lin["cost"]
    while True:
        st["cost_final"], st["grad_max"], st["lambda_final"] = lin["cost"], float(np.abs(lin["g"]).max()), lam
        if st["grad_max"] <= params["gtol"]:
            st["stop_reason"] = STOP_GRADIENT
            break
        if st["outer"] == params["max_outer"]:
            st["stop_reason"] = STOP_MAX_OUTER
            break
        st["outer"] += 1
        H, free = dense_system(graph, lin)
        Hff = H[np.ix_(free, free)]
        Dff = np.diag(Hff).copy()
        A = Hff + lam * np.diag(Dff)
        gf = lin["g"].reshape(-1)[free]
        df = np.linalg.solve(A, -gf)
        if count_pcg:
            _, its, capped = pcg(A, -gf, params["pcg_rtol"], params["max_pcg"])
            st["pcg_iters"].append(its)
            st["pcg_capped"] += int(capped)
        d = np.zeros(6 * n)
        d[free] = df
        d = d.reshape(n, 6)
        cand = retract(poses, d, fixed)
        cost_new = cost_of(graph, cand)
        denom = float(df @ (lam * Dff * df - gf))
        accepted, lam, nu, _ = lm_policy(lin["cost"], cost_new, denom, lam, nu)
        st["lambda_final"] = lam
        if accepted:
            poses = cand
            st["accepted"] += 1
            lin = linearise(graph, poses)
        if np.abs(df).max() <= params["xtol"]:
            st["stop_reason"] = STOP_STEP
            st["cost_final"], st["grad_max"] = lin["cost"], float(np.abs(lin["g"]).max())
            break
    return poses, st


# ---- graphs -----------------------------------------------------------------------------------------------------------
def compose(X, Y):
    """X * Y for poses (..., 7)"""
    R = quat_R(X[..., 3:])
    t = X[..., :3] + (R @ Y[..., :3, None])[..., 0]
    q = quat_mul(X[..., 3:], Y[..., 3:])
    return np.concatenate([t, q / np.linalg.norm(q, axis=-1, keepdims=True)], axis=-1)


def between(Xi, Xj):
    """the pose of j in i's frame"""
    RiT = np.swapaxes(quat_R(Xi[..., 3:]), -1, -2)
    t = (RiT @ (Xj[..., :3] - Xi[..., :3])[..., None])[..., 0]
    qi = Xi[..., 3:] * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([t, quat_mul(qi, Xj[..., 3:])], axis=-1)


def random_spd(rng, m):
    """m SPD 6x6: rotation information around 1e4, translation around 2.5e3, mixed, condition number below 100"""
    A = rng.normal(size=(m, 6, 6))
    core = np.eye(6) + 0.3 * (A @ np.swapaxes(A, -1, -2)) / 6.0
    S = np.array([100.0] * 3 + [50.0] * 3)
    Om = S[None, :, None] * core * S[None, None, :]
    return 0.5 * (Om + np.swapaxes(Om, -1, -2))


def ring_with_spokes(n, seed, delta=0.0, second_hub=False, noise=True, spoke_every=3):
    """n poses on a 20 m circle, rising 0.1 m per node, with random tilt; an odometry edge k -> k + 1 and the closing edge
    n - 1 -> 0; spokes 0 -> k for every `spoke_every`-th k (and, with second_hub, from node n // 2 as well); measurement
    noise 0.01 rad / 0.02 m (none with noise=False); a random SPD Omega per edge; the initial guess dead-reckoned from the
    odometry measurements with a yaw bias of 0.004 rad and 0.03 m per step; node 0 fixed.  Also returns the ground truth."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / max(n, 1)
    t = np.stack([20 * np.cos(ang), 20 * np.sin(ang), 0.1 * np.arange(n)], axis=-1)
    yaw = quat_exp(np.stack([np.zeros(n), np.zeros(n), ang + np.pi / 2], axis=-1))
    truth = np.concatenate([t, quat_mul(yaw, quat_exp(0.05 * rng.normal(size=(n, 3))))], axis=-1)
    ij = [(k, k + 1) for k in range(n - 1)]
    if n > 2:
        ij.append((n - 1, 0))
    ij += [(0, k) for k in range(2, n - 1, spoke_every)]
    if second_hub:
        h = n // 2
        ij += [(h, k) for k in range(1, n, spoke_every) if abs(k - h) > 1]
    ij = np.array(ij, np.int32).reshape(-1, 2)
    m = len(ij)
    Z = between(truth[ij[:, 0]], truth[ij[:, 1]]) if m else np.zeros((0, 7))
    if noise and m:
        nz = np.concatenate([0.02 * rng.normal(size=(m, 3)), quat_exp(0.01 * rng.normal(size=(m, 3)))], axis=-1)
        Z = compose(Z, nz)
    guess = truth.copy()
    bias = np.concatenate([[0.03, 0, 0], quat_exp(np.array([0, 0, 0.004]))])
    for k in range(1, n):
        guess[k] = compose(compose(guess[k - 1], Z[k - 1]), bias)
    fixed = np.zeros(n, bool)
    fixed[:1] = True
    graph = {"poses": guess, "fixed": fixed, "ij": ij, "Z": Z, "Om": random_spd(rng, m),
             "delta": np.full(m, float(delta))}
    return graph, truth


def pose_delta(a, b):
    """largest translation and rotation distance between two pose arrays"""
    dt = np.linalg.norm(a[:, :3] - b[:, :3], axis=1).max()
    dq = np.abs(np.einsum("na,na->n", a[:, 3:], b[:, 3:])).clip(0, 1)
    return float(dt), float((2 * np.arccos(dq)).max())
