"""The C++ mirror of the batched quality report's host functions (include/lidar_odometry_amd.hpp: lom::poseLattice,
CloudMatcher::bestQuality, and that CloudMatcher::qualityBatch compiles): tests/cpp/test_quality_batch.cpp, compiled by
plain g++ as tests/test_quality_cpp.py does, checks them against the C functions.  Host code only: no GPU needed."""
from tests import cpp_program


def test_cpp_mirror_quality_batch(tmp_path, lom):
    exe = cpp_program.build_with_library(tmp_path, "test_quality_batch.cpp")
    cpp_program.run(exe, timeout=300)
