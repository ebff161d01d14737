"""The C++ mirror of place recognition (include/lidar_odometry_amd.hpp: lom::PlaceDatabase, LidarOdometry::placeDescriptor):
tests/cpp/test_place.cpp, compiled by plain g++ as tests/test_quality_batch_cpp.py does, checks shiftYaw and the refusals
against the C functions.  Host code only: no GPU needed."""
import os
import subprocess

from tests.conftest import ROOT


def test_cpp_mirror_place(tmp_path, lom):
    exe = str(tmp_path / "test_place")
    libdir = os.path.join(ROOT, "lidar_odometry_demo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_place.cpp"), "-o", exe, "-L", libdir,
                           "-llidar_odometry_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL PASSED" in r.stdout
