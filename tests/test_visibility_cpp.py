"""The visibility grid's host planning under sanitizers: tests/cpp/test_visibility.cpp compiles csrc/visibility_host.cpp --
value checks, the direction table, window sizes, launch shapes, the selection key's bit budget -- under
-fsanitize=address,undefined into a program of its own, with no HIP header on its include path.  Host code only: no GPU
needed, and nothing is loaded into Python."""
from tests import cpp_program


def test_visibility_host_under_sanitizers(tmp_path):
    cpp_program.run(cpp_program.build_host(tmp_path, "test_visibility.cpp", ["visibility_host.cpp"]), timeout=300)
