"""The clearance grid's host planning under sanitizers: tests/cpp/test_clearance.cpp compiles csrc/clearance_host.cpp --
value ranges, the radius in cells, the cost table, the clipped and grown rectangles, the launch shapes of the two kernels
-- under -fsanitize=address,undefined into a program of its own, with no HIP header on its include path.  Host code only:
no GPU needed, and nothing is loaded into Python."""
from tests import cpp_program


def test_clearance_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_clearance.cpp", ["clearance_host.cpp"])
    cpp_program.run(exe, timeout=300)
