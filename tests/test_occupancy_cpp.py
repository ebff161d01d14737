"""The host planner of the occupancy grid under sanitizers: tests/cpp/test_occupancy.cpp with -DOCCUPANCY_HOST_STANDALONE
compiles csrc/occupancy_host.cpp and csrc/assemble_host.cpp themselves under -fsanitize=address,undefined into a program of
its own -- every refusal, the slices of 1, 63, 64, 65 and 129 scans, bounding boxes clipped at the grid's edges and for
origins outside it, the step bound, the scratch-budget slice size.  Host code only: no GPU needed, and nothing is loaded
into Python."""
from tests import cpp_program


def test_occupancy_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_occupancy.cpp", ["occupancy_host.cpp", "assemble_host.cpp"],
                                 ["-DOCCUPANCY_HOST_STANDALONE", "-I", cpp_program.INCLUDE])
    cpp_program.run(exe, timeout=300)
