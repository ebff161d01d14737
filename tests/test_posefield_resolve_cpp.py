"""The host planning of the pose field's re-solve under sanitizers: tests/cpp/test_posefield_resolve.cpp compiles
csrc/posefield_host.cpp (with csrc/navfield_host.cpp and csrc/visibility_host.cpp, as tests/test_posefield_cpp.py does) and
checks posefield::relayer_boxes -- the eight boxes k_pose_relayer runs over -- against a brute-force dilation, under
-fsanitize=address,undefined in a program of its own with no HIP header on its include path.  The C++ mirror's three
re-solve methods compile and the refusals that need no device run.  Host code only: no GPU needed, and nothing is loaded into
Python."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")


def test_relayer_boxes_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_posefield_resolve")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_posefield_resolve.cpp"),
                           os.path.join(CSRC, "posefield_host.cpp"), os.path.join(CSRC, "navfield_host.cpp"),
                           os.path.join(CSRC, "visibility_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout


def test_cpp_mirror_compiles_and_its_refusals_run(tmp_path):
    exe = str(tmp_path / "test_posefield_resolve_mirror")
    libdir = os.path.join(ROOT, "lidar_odometry_demo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_posefield_resolve_mirror.cpp"), "-o", exe, "-L", libdir,
                           "-llidar_odometry_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
