"""The region grid's host planning under sanitizers: tests/cpp/test_regions.cpp compiles csrc/regions_host.cpp -- value
checks, word, tile and lane counts, the centroid rounding, the list sort -- under -fsanitize=address,undefined into a
program of its own, with no HIP header on its include path.  Host code only: no GPU needed, and nothing is loaded into
Python."""
from tests import cpp_program


def test_regions_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_regions.cpp", ["regions_host.cpp"])
    cpp_program.run(exe, timeout=300)
