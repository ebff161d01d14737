"""The re-solve of the pose field restated on Python integers (include/lidar_odometry_amd.h, "pose field", "Re-solve"), on
top of tests/posefield_ref.py: the merged plane, the derived goal states, the changed states, the least raised set over
states by the safety rule, and the relaxation of what is left.  resolve() gives what the device must leave: the full solve of
the merged plane for the derived goal states, with the counts of the diff, of the layers and of the raise phase.  A state is
the index h * cells + y * width + x, as in posefield_ref.edges_of."""
import heapq

import numpy as np

from tests import navfield_resolve_ref as NR
from tests import posefield_ref as R

U = R.UNREACHED
clip, merged_plane, changed_cells = NR.clip, NR.merged_plane, NR.changed_cells


def derived_goals(P):
    """the states with P == 0, as (ix, iy, h) rows"""
    return np.argwhere(np.asarray(P) == 0)[:, ::-1].astype(np.int32).reshape(-1, 3)


def changed_states(L_old, L_new):
    """the (h, y, x) whose layer differs"""
    return np.argwhere(np.asarray(L_old, np.int64) != np.asarray(L_new, np.int64))


def as_list(P):
    return [int(v) for v in np.asarray(P).reshape(-1)]


def drop_impassable(P, L):
    """the layers' part: a reached state whose layer is 0 reads unreached; returns how many"""
    flat = np.asarray(L).reshape(-1)
    n = 0
    for u, p in enumerate(P):
        if p != U and not flat[u]:
            P[u] = U
            n += 1
    return n


def out_moves(n_states, src, tgt, wgt):
    """the allowed moves by source state: (first, targets, weights) with the moves of u at first[u] .. first[u + 1]"""
    order = np.argsort(src, kind="stable")
    return np.searchsorted(src[order], np.arange(n_states + 1)).tolist(), tgt[order].tolist(), wgt[order].tolist()


def least_raised_set(P, edges):
    """The raise phase on a list of Python integers P (impassable states unreached already), in place: in increasing order of
    P, a reached state a with P[a] > 0 stays iff some allowed move a -> b has P[b] reached and P[b] + weight <= P[a].  Every
    weight is positive, so supporters have strictly lower P, and when a state's turn comes its supporters are final.
    Returns the set of states that rose."""
    first, to, wt = out_moves(len(P), *edges)
    rose = set()
    for p, u in sorted((p, u) for u, p in enumerate(P) if p != U and p > 0):
        if not any(P[to[k]] != U and P[to[k]] + wt[k] <= p for k in range(first[u], first[u + 1])):
            P[u] = U
            rose.add(u)
    return rose


def raised_by_definition(P, edges):
    """The same set by the definition alone: set every unsafe state unreached, again and again, until none is left"""
    first, to, wt = out_moves(len(P), *edges)
    rose = set()
    while True:
        unsafe = [u for u, p in enumerate(P) if p != U and p > 0 and
                  not any(P[to[k]] != U and P[to[k]] + wt[k] <= p for k in range(first[u], first[u + 1]))]
        if not unsafe:
            return rose
        for u in unsafe:
            P[u] = U
        rose.update(unsafe)


def relax(P, edges):
    """the relaxation from upper bounds, in place, to its fixed point: a heap over every reached state"""
    src, tgt, wgt = edges
    order = np.argsort(tgt, kind="stable")
    first = np.searchsorted(tgt[order], np.arange(len(P) + 1)).tolist()
    back, wb = src[order].tolist(), wgt[order].tolist()
    heap = [(p, u) for u, p in enumerate(P) if p != U]
    heapq.heapify(heap)
    while heap:
        d, u = heapq.heappop(heap)
        if d != P[u]:
            continue
        for k in range(first[u], first[u + 1]):
            cand = d + wb[k]
            if cand <= R.MAX and cand < P[back[k]]:
                P[back[k]] = cand
                heapq.heappush(heap, (cand, back[k]))


def to_array(P, shape):
    return np.array(P, dtype=np.uint64).astype(np.uint32).reshape(shape)


def raise_then_relax(P_old, L_new, p):
    """The incremental form on the reference: (P uint32, the states that rose)"""
    L = np.asarray(L_new, np.int64)
    edges = R.edges_of(L, p)
    P = as_list(P_old)
    drop_impassable(P, L)
    rose = least_raised_set(P, edges)
    relax(P, edges)
    return to_array(P, L.shape), rose


def resolve(geo, kept, new, window, p, footprint, ref_old):
    """What a re-solve must leave, from what the last solve or re-solve left (ref_old: its L and P): the dict of
    posefield_ref.solve of the merged plane for the derived goal states, and with it plane (the merged plane), cells_changed,
    states_changed, states_raised (the size of the least raised set) and P_raised (P behind the raise phase, before the
    relaxation)."""
    merged = merged_plane(kept, new, window)
    out = R.solve(geo, merged, p, footprint, derived_goals(ref_old["P"]))
    assert not out["error"]
    L = out["L"].astype(np.int64)
    P = as_list(ref_old["P"])
    drop_impassable(P, L)
    rose = least_raised_set(P, R.edges_of(L, p))
    out.update(plane=merged, cells_changed=len(changed_cells(kept, merged)), states_changed=len(changed_states(ref_old["L"], L)),
               states_raised=len(rose), P_raised=to_array(P, L.shape))
    return out
