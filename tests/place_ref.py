"""numpy reference of the place-recognition definitions (include/lidar_odometry_amd.h, "place recognition"), written
from those definitions alone, in f64, independent of the product, plus the seeded scenes the tests use.

Tolerance on a distance, derived not measured
---------------------------------------------
The device stores unit columns in f32 and forms d(s) in f32; with u = 2^-24:
  * a unit column in f32 carries at most (R/2 + 2) u per column (the norm's sum of R squares, the square root, the
    division, the rounding to f32);
  * a dot product of R terms of two unit vectors carries R u (the standard gamma_n bound with Cauchy-Schwarz:
    sum |q_r c_r| <= 1);
  * the mean over at most S columns in f32 carries S u, plus the division and the subtraction from 1.
Two unit columns, one dot product, the mean and the last two operations:  TOL = (2R + S + 10) * 2^-24, which is
6.6e-6 at 20 x 60.  The product computes its column norms in f64, which is inside this bound; TOL is not loosened.
"""
import numpy as np

TWO_PI = 2.0 * np.pi


def tol(R, S):
    return (2 * R + S + 10) * 2.0 ** -24


def _params(params):
    R, S, max_range, z_floor = params
    return int(R), int(S), np.float32(max_range), np.float32(z_floor)


def describe(xyz, params):
    """(descriptor (R, S) f32, ill (n,) bool).  `ill` marks the points whose rho / ring width or phi / sector width
    lies within 1e-9 of an integer: those whose cell may legitimately differ by one between two correct sqrt / atan2
    implementations."""
    R, S, max_range, z_floor = _params(params)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if not np.isfinite(xyz).all():
        raise ValueError("non-finite coordinate")  # LOM_ERR_RANGE
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    t = np.sqrt(x * x + y * y) / (np.float64(max_range) / R)
    ring = np.floor(t)
    phi = np.arctan2(y, x)
    phi = np.where(phi < 0.0, phi + TWO_PI, phi)
    a = phi / (TWO_PI / S)
    sector = np.floor(a).astype(np.int64)
    sector[sector >= S] = 0  # phi + 2 pi rounded to 2 pi itself: the angle 0
    v = xyz[:, 2] - z_floor  # one f32 subtraction
    assert v.dtype == np.float32
    keep = (ring < R) & (v > 0)
    desc = np.zeros((R, S), np.float32)
    np.maximum.at(desc, (ring[keep].astype(np.int64), sector[keep]), v[keep])
    ill = (np.abs(t - np.round(t)) < 1e-9) | (np.abs(a - np.round(a)) < 1e-9)
    return desc, ill


def _unit(d):
    d = np.asarray(d, np.float64)
    n = np.sqrt((d * d).sum(axis=-2, keepdims=True))
    nz = n > 0
    return np.where(nz, d / np.where(nz, n, 1.0), 0.0), nz.squeeze(-2)


def distances_many(q, entries):
    """d(s) of one query (R, S) against entries (N, R, S): an (N, S) f64 array."""
    qu, qm = _unit(q)
    cu, cm = _unit(entries)
    S = qu.shape[-1]
    M = np.einsum("rj,nrk->njk", qu, cu)          # cos(q_j, c_k)
    both = qm[None, :, None] & cm[:, None, :]
    j = np.arange(S)
    out = np.ones((cu.shape[0], S))
    for s in range(S):
        k = (j + s) % S
        cnt = both[:, j, k].sum(axis=1)
        tot = np.where(both[:, j, k], M[:, j, k], 0.0).sum(axis=1)
        out[:, s] = np.where(cnt > 0, 1.0 - tot / np.maximum(cnt, 1), 1.0)
    return out


def distances(q, c, params=None):
    """all S values of d(s) for one pair"""
    return distances_many(q, np.asarray(c)[None])[0]


def best_shift(ds):
    """(distance, shift) per row of an (N, S) array: the minimum over s, the smallest s on a tie"""
    s = np.argmin(ds, axis=1)
    return ds[np.arange(len(ds)), s], s


def query(qs, entries, k, id_begin=0, id_end=None):
    """The ranking rule: per query the k entries of [id_begin, id_end) with the smallest (distance, id); empty slots
    hold id -1, distance inf, shift 0.  Returns (ids (Q, k) i8, dist (Q, k) f8, shift (Q, k) i8, all_dist (Q, n) f8)."""
    qs = np.asarray(qs)
    qs = qs[None] if qs.ndim == 2 else qs
    entries = np.asarray(entries)
    id_end = len(entries) if id_end is None else id_end
    n = id_end - id_begin
    ids = np.full((len(qs), k), -1, np.int64)
    dist = np.full((len(qs), k), np.inf)
    shift = np.zeros((len(qs), k), np.int64)
    alld = np.ones((len(qs), n))
    for qi, q in enumerate(qs):
        if n == 0:
            continue
        d, s = best_shift(distances_many(q, entries[id_begin:id_end]))
        alld[qi] = d
        order = np.argsort(d, kind="stable")[:k]  # stable: equal distances go to the smaller id
        ids[qi, :len(order)] = order + id_begin
        dist[qi, :len(order)] = d[order]
        shift[qi, :len(order)] = s[order]
    return ids, dist, shift, alld


# ---- scenes, in polar form so that structure is controlled -------------------------------------------------------

def _field(rng, R, S):
    """a smooth height field over (ring, sector), periodic in the sector"""
    rr, ss = np.meshgrid(np.arange(R) / max(R, 1), np.arange(S) / max(S, 1), indexing="ij")
    h = np.full((R, S), 1.5)
    for _ in range(6):
        fr, fs = rng.integers(0, 3), rng.integers(1, 5)
        h = h + rng.uniform(0.3, 1.0) * np.cos(TWO_PI * (fr * rr + fs * ss) + rng.uniform(0, TWO_PI))
    return h


def scene_cloud(seed, params, n=4000, rotate_sectors=0, noise_seed=None):
    """About n points: a seeded smooth height field plus noise, an angular density modulation, points beyond max_range
    and below z_floor among them.  Every point sits at least 2 % of a cell away from its cell's borders, so no point is
    `ill` and a rotation by whole sectors moves whole columns.  rotate_sectors adds k 2 pi / S to theta before the
    conversion to f32 xyz.  noise_seed: other noise and sampling on the same field."""
    R, S, max_range, z_floor = _params(params)
    rng = np.random.default_rng(seed)
    h = _field(rng, R, S)
    dens = 0.55 + 0.45 * np.cos(TWO_PI * np.arange(S) / S * rng.integers(1, 4) + rng.uniform(0, TWO_PI))
    if noise_seed is not None:
        rng = np.random.default_rng([seed, noise_seed])
    sector = rng.choice(S, size=n, p=dens / dens.sum())
    ring = rng.integers(0, R + max(R // 8, 1), size=n)  # the last rings lie beyond max_range
    rho = (ring + rng.uniform(0.02, 0.98, n)) * (float(max_range) / R)
    theta = (sector + rng.uniform(0.02, 0.98, n) + rotate_sectors) * (TWO_PI / S)
    z = float(z_floor) + h[np.minimum(ring, R - 1), sector] + rng.normal(0, 0.4, n)  # some end below z_floor
    return np.stack([rho * np.cos(theta), rho * np.sin(theta), z], axis=1).astype(np.float32)


def scene_descriptor(seed, params, like=None, noise=0.05):
    """A descriptor straight from the generator (what a cloud of such a scene describes to, at cell granularity): the
    field plus noise, clipped at 0, some columns and cells empty.  like=(descriptor, shift): a noisy copy of another
    one, its columns moved by `shift`."""
    R, S, _, _ = _params(params)
    rng = np.random.default_rng([seed, 77])
    if like is not None:
        base, shift = like
        d = np.roll(np.asarray(base, np.float64), shift, axis=1)
        d = np.where(d > 0, np.maximum(d + rng.normal(0, noise, d.shape), 0.0), 0.0)
        return d.astype(np.float32)
    d = np.maximum(_field(rng, R, S) + rng.normal(0, 0.4, (R, S)), 0.0)
    d[rng.random((R, S)) < 0.1] = 0.0
    d[:, rng.random(S) < 0.08] = 0.0
    return d.astype(np.float32)


def check_conditions(qs, entries, params, k, ranges):
    """The conditions a scene set must meet before the GPU is asked about it; returns the list of violations (empty:
    the set is fit).  For every query and every id range used: every gap between the best and second-best shift of a
    pair above 4 TOL, and every gap between consecutive ranked entries among the first k + 1 above 4 TOL."""
    R, S = int(params[0]), int(params[1])
    lim = 4 * tol(R, S)
    bad = []
    for qi, q in enumerate(qs):
        ds = distances_many(q, entries)
        if S > 1:
            two = np.sort(ds, axis=1)[:, :2]
            for e in np.nonzero(two[:, 1] - two[:, 0] <= lim)[0]:
                bad.append(("shift", qi, int(e)))
        d = ds.min(axis=1)
        for b, e in ranges:
            order = np.argsort(d[b:e], kind="stable")[:k + 1] + b
            gaps = np.diff(d[order])
            for g in np.nonzero(gaps <= lim)[0]:
                bad.append(("rank", qi, int(order[g + 1])))
    return bad


def fit_database(params, queries, n, k, ranges, seed=1000, protect=()):
    """n entry descriptors from the generator that meet check_conditions for `queries`: candidates come in seed order,
    and one that breaks a condition is dropped (the reference decides the scenes).  `protect`: entries placed first, as
    they are (never dropped: a set they spoil is a failure of the caller's)."""
    entries = [np.asarray(p, np.float32) for p in protect]
    next_seed = seed
    while True:
        while len(entries) < n:
            entries.append(scene_descriptor(next_seed, params))
            next_seed += 1
        bad = check_conditions(queries, np.stack(entries), params, k, [(b, min(e, n)) for b, e in ranges])
        drop = sorted({e for _, _, e in bad if e >= len(protect)}, reverse=True)
        if not drop:
            return np.stack(entries), bad
        for e in drop:
            del entries[e]


# ---- the sets the host test checks and the GPU test uses -----------------------------------------------------------

PARAMS = (20, 60, 80.0, -1.5)
PARAMS_BIG = (64, 64, 100.0, -2.0)
# k_place_query works on groups of 8 entries and tiles of 64: either side of both, and many tiles
QUERY_SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 1000)
SUB_RANGE = (13, 500)
_cache = {}


def query_set(params=PARAMS, n=1000, sizes=QUERY_SIZES, sub_range=SUB_RANGE):
    """(queries (3, R, S), entries (n, R, S), violations): three queries -- noisy, turned copies of entries 0 and 1,
    and a scene of its own -- and a database fitted to them for every prefix in `sizes` and for `sub_range`, k = 64."""
    key = (params, n, sizes, sub_range)
    if key not in _cache:
        b0, b1 = scene_descriptor(1, params), scene_descriptor(2, params)
        S = int(params[1])
        qs = np.stack([scene_descriptor(11, params, like=(b0, 11 % S)), scene_descriptor(12, params, like=(b1, 29 % S)),
                       scene_descriptor(13, params)])
        ranges = [(0, s) for s in sizes if s <= n] + ([sub_range] if sub_range and sub_range[1] <= n else [])
        entries, bad = fit_database(params, qs, n, 64, ranges, protect=(b0, b1))
        _cache[key] = (qs, entries, bad)
    return _cache[key]
