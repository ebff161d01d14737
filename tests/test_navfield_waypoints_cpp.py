"""Steps 8 and 9 of the navigation field on the host under sanitizers: tests/cpp/test_navfield_waypoints.cpp compiles
csrc/nav_los_rule.hpp -- the rule the kernels run -- and csrc/navfield_host.cpp under -fsanitize=address,undefined into a
program of its own, with no HIP header on its include path, runs it on planes, pairs and routes written here, and its
answers equal tests/navfield_waypoints_ref.py's byte for byte.  Host code only: no GPU needed, nothing loaded into Python."""
import numpy as np

from tests import cpp_program
from tests import navfield_ref as N
from tests import navfield_scenes as S
from tests import navfield_waypoints_ref as Wr

P0 = N.params(50, 3, 400, 98)
P1 = N.params(50, 3, 400, 90, N.UNKNOWN_PASSABLE)


def cases():
    """(w, h, plane, params, max_cell_cost, lookahead, wp_cap, pairs, routes)"""
    rng = np.random.default_rng(77)
    out = []
    for w, h, plane, p in ((1, 1, S.empty(1, 1), P0), (1, 9, S.empty(1, 9), P0), (13, 1, S.empty(13, 1), P0),
                           (13, 11, S.random_plane(rng, 13, 11, obstacles=0.15), P1), (33, 31, S.random_plane(rng, 33, 31, obstacles=0.1), P0),
                           (40, 40, S.diagonal_gaps(40, 40), P0), (30, 20, S.pocket(30, 20), P0), (25, 25, S.spiral(25, 25), P0),
                           (70, 9, S.empty(70, 9), P0)):
        geo = N.geometry(0.25, 0.0, 0.0, w, h)
        free = np.argwhere((plane >= 0) & (plane <= 90))       # passable under both parameter sets
        r = N.solve(geo, plane, p, free[:1, ::-1])
        starts = [tuple(int(v) for v in free[i][::-1]) for i in rng.integers(0, len(free), 6)] + [(w - 1, h - 1), (0, 0)]
        routes = [N.path(geo, r["costs"], r["P"], s) for s in starts] + [[]]
        pairs = np.stack([rng.integers(-1, w + 1, 150), rng.integers(-1, h + 1, 150), rng.integers(-1, w + 1, 150),
                          rng.integers(-1, h + 1, 150)], axis=1).astype(np.int32)
        for mcc, W, wp_cap in ((0, 65535, 64), (50, 3, 2), (80, 64, 0)):
            out.append((w, h, plane, p, mcc, W, wp_cap, pairs, routes))
    return out


def test_rule_and_planner_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_navfield_waypoints.cpp", ["navfield_host.cpp"])
    all_cases = cases()
    blob, want = [np.uint32(len(all_cases)).tobytes()], []
    n_visible = n_cut = 0
    for w, h, plane, p, mcc, W, wp_cap, pairs, routes in all_cases:
        c = N.costs_of(plane, p)
        blob.append(np.array([w, h, mcc, W, wp_cap, len(pairs), len(routes)], np.uint32).tobytes())
        blob.append(np.array(N.cell_costs(p), np.uint32).tobytes())
        blob.append(np.ascontiguousarray(plane, np.int8).tobytes())
        blob.append(pairs.tobytes())
        vis = Wr.visible_many(c, w, h, pairs, mcc)
        n_visible += int(vis.sum())
        want.append(vis.tobytes())
        for route in routes:
            blob.append(np.uint32(len(route)).tobytes() + np.array(route, np.uint16).reshape(-1, 2).tobytes())
            wp = Wr.shortcut(route, W, lambda a, b: Wr.visible(c, w, h, a, b, mcc))
            n_cut += len(wp) < len(route)
            cells = np.zeros((wp_cap, 2), np.uint16)
            head = np.array(wp[:wp_cap], np.uint16).reshape(-1, 2)
            cells[:len(head)] = head
            want.append(np.uint32(len(wp)).tobytes() + cells.tobytes())
    assert n_visible > 200 and n_cut > 20                   # the cases say something
    src, dst = tmp_path / "cases.bin", tmp_path / "answers.bin"
    src.write_bytes(b"".join(blob))
    cpp_program.run(exe, str(src), str(dst), timeout=300)
    assert dst.read_bytes() == b"".join(want)
