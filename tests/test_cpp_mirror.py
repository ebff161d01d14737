"""The header-only C++ mirror (include/lidar_odometry_amd.hpp) of the reference classes:
compiles with plain g++ against the C ABI (CPU check) and passes the reference's gtest
cases restated in tests/cpp/test_mirror.cpp (GPU check)."""
import os

import pytest

from tests import cpp_program


def test_mirror_header_compiles_and_links(tmp_path, lom):
    assert os.path.exists(cpp_program.build_with_library(tmp_path, "test_mirror.cpp"))


@pytest.mark.gpu
def test_mirror_passes_reference_cases(tmp_path, lom):
    cpp_program.run(cpp_program.build_with_library(tmp_path, "test_mirror.cpp"), timeout=300)
