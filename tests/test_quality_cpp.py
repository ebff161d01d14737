"""The C++ mirror of the quality report (include/lidar_odometry_amd.hpp: lom::QualityReport, CloudMatcher::quality,
LidarOdometry::setQualityReport / getQuality): tests/cpp/test_quality.cpp, compiled by plain g++ as tests/test_cpp_mirror.py
does, checks them against the C ABI on the GPU."""
import pytest

from tests import cpp_program

pytestmark = pytest.mark.gpu


def test_cpp_mirror_quality(tmp_path, lom):
    cpp_program.run(cpp_program.build_with_library(tmp_path, "test_quality.cpp"), timeout=300)
