"""The host planner of the elevation grid under sanitizers: tests/cpp/test_elevation.cpp with -DELEVATION_HOST_STANDALONE
compiles csrc/elevation_host.cpp and csrc/assemble_host.cpp themselves under -fsanitize=address,undefined into a program of
its own -- every value range, the origins' start cells and range verdict, every refusal of the planner in the definition's
order, launches under a cap, empty scans and an empty call.  Host code only: no GPU needed, and nothing is loaded into
Python."""
from tests import cpp_program


def test_elevation_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_elevation.cpp", ["elevation_host.cpp", "assemble_host.cpp"],
                                 ["-DELEVATION_HOST_STANDALONE", "-I", cpp_program.INCLUDE])
    cpp_program.run(exe, timeout=300)
