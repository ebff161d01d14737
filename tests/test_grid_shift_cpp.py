"""The rule of the grid shift on the host under sanitizers: tests/cpp/test_grid_shift.cpp compiles csrc/plane_geometry.hpp --
the rule every handle's shift takes -- and its C ABI, csrc/grid_shift_host.cpp, under -fsanitize=address,undefined into a
program of its own, with no HIP header on its include path and against the C++ mirror's new members, and runs it directly
over the table of cases of tests/test_grid_shift_host.py: the answers are tests/grid_shift_ref.py's.  Host code only: no GPU
needed, nothing loaded into Python."""
import struct

import numpy as np

from tests import cpp_program
from tests import grid_shift_ref as R
from tests.test_grid_shift_host import DYADIC, EDGE, EDGE_CASES, SHIFTS, TENTH, admissible


def shift_cases():
    """(geometry, dx, dy): the table of test_shift_geometry_bits and test_shift_geometry_refusals"""
    out = [(g, dx, dy) for g in (DYADIC, TENTH) for dx in SHIFTS for dy in SHIFTS]
    big = dict(resolution=1e30, origin_x=3e38, origin_y=0.0, width=8, height=8)
    out += [(big, 1000000000, 0), (big, R.I32_MAX, 0), (big, -100000000, 0), (dict(big, origin_x=0.0, origin_y=3e38), 0, R.I32_MAX),
            (dict(big, origin_x=0.0, origin_y=-3e38), 0, R.I32_MIN)]
    out += [(EDGE, dx, dy) for dx, dy, _ in EDGE_CASES]           # a quarter and a half of an ulp beyond FLT_MAX
    nan, inf = float("nan"), float("inf")
    out += [(g, 1, 1) for g in (dict(DYADIC, resolution=0.0), dict(DYADIC, resolution=-0.25), dict(DYADIC, resolution=nan),
                                dict(DYADIC, resolution=inf), dict(DYADIC, origin_x=nan), dict(DYADIC, origin_y=-inf),
                                dict(DYADIC, width=0), dict(DYADIC, height=0), dict(DYADIC, width=16385), dict(DYADIC, height=16385),
                                dict(DYADIC, width=16384, height=16384))]
    return out


def test_rule_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_grid_shift.cpp", ["grid_shift_host.cpp"], ["-ffp-contract=off", "-I", cpp_program.INCLUDE])
    cases = shift_cases()
    blob = [np.uint32(len(cases)).tobytes()]
    for g, dx, dy in cases:
        status, want = R.shift_geometry(g, dx, dy)
        wx, wy = (want["origin_x"], want["origin_y"]) if status == R.OK else (0.0, 0.0)
        blob.append(struct.pack("<fffIIiiiff", g["resolution"], g["origin_x"], g["origin_y"], g["width"], g["height"], dx, dy, status,
                                wx, wy))
    q = np.arange(-200, 240, dtype=np.int64)
    n_rows = 0
    for n in range(2, 41):
        for margin, quantum in admissible(n):                 # quantum-major, as the program walks them
            blob.append(R.follow_cells(q, n, margin, quantum).astype(np.int32).tobytes())
            n_rows += 1
    assert n_rows == 2870
    src = tmp_path / "cases.bin"
    src.write_bytes(b"".join(blob))
    assert "follow calls: 2525600" in cpp_program.run(exe, str(src), timeout=300)
