"""The navigation field's host planning under sanitizers: tests/cpp/test_navfield.cpp compiles csrc/navfield_host.cpp --
value ranges, the cell-cost table, goal quantisation at cell borders and grid edges, tile counts -- under
-fsanitize=address,undefined into a program of its own, with no HIP header on its include path.  Host code only: no GPU
needed, and nothing is loaded into Python."""
from tests import cpp_program


def test_navfield_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_navfield.cpp", ["navfield_host.cpp"])
    cpp_program.run(exe, timeout=300)
