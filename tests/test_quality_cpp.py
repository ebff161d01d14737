"""The C++ mirror of the quality report (include/lidar_odometry_amd.hpp: lom::QualityReport, CloudMatcher::quality,
LidarOdometry::setQualityReport / getQuality): tests/cpp/test_quality.cpp, compiled by plain g++ as tests/test_cpp_mirror.py
does, checks them against the C ABI on the GPU."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_mirror_quality(tmp_path, lom):
    exe = str(tmp_path / "test_quality")
    libdir = os.path.join(ROOT, "lidar_odometry_demo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_quality.cpp"), "-o", exe, "-L", libdir,
                           "-llidar_odometry_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL PASSED" in r.stdout
