"""The C++ mirror of place recognition (include/lidar_odometry_amd.hpp: lom::PlaceDatabase, LidarOdometry::placeDescriptor):
tests/cpp/test_place.cpp, compiled by plain g++ as tests/test_quality_batch_cpp.py does, checks shiftYaw and the refusals
against the C functions.  Host code only: no GPU needed."""
from tests import cpp_program


def test_cpp_mirror_place(tmp_path, lom):
    exe = cpp_program.build_with_library(tmp_path, "test_place.cpp")
    cpp_program.run(exe, timeout=300)
