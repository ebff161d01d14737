"""The C++ side of the pose graph: tests/cpp/test_graph.cpp is compiled twice by plain g++.  Against the library it checks
the mirror lom::PoseGraph (include/lidar_odometry_amd.hpp) and the stateless host functions; with -DGRAPH_HOST_STANDALONE
it compiles csrc/graph_host.cpp itself under -fsanitize=address,undefined into a program of its own and runs the gauge
check, the CSR build and the Cholesky on degenerate shapes.  Host code only: no GPU needed."""
from tests import cpp_program


def test_cpp_mirror_graph(tmp_path, lom):
    cpp_program.run(cpp_program.build_with_library(tmp_path, "test_graph.cpp"), timeout=300)


def test_graph_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_graph.cpp", ["graph_host.cpp"], ["-DGRAPH_HOST_STANDALONE", "-I", cpp_program.INCLUDE])
    cpp_program.run(exe, timeout=300)
