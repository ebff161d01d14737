"""The C++ side of the scan archive and the map assembly: tests/cpp/test_assemble.cpp is compiled twice by plain g++.
Against the library it checks the mirror lom::ScanArchive / VoxelGrid::assemble (include/lidar_odometry_amd.hpp) and the
host function; with -DASSEMBLE_HOST_STANDALONE it compiles csrc/assemble_host.cpp itself under
-fsanitize=address,undefined into a program of its own and runs the planner on degenerate and extreme inputs.  Host code
only: no GPU needed (with one, the first program also assembles a small map)."""
from tests import cpp_program


def test_cpp_mirror_assemble(tmp_path, lom):
    exe = cpp_program.build_with_library(tmp_path, "test_assemble.cpp")
    cpp_program.run(exe, timeout=300)


def test_assemble_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_assemble.cpp", ["assemble_host.cpp"],
                                 ["-DASSEMBLE_HOST_STANDALONE", "-I", cpp_program.INCLUDE])
    cpp_program.run(exe, timeout=300)
