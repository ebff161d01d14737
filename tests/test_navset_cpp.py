"""The navigation field set's host planning under sanitizers: tests/cpp/test_navset.cpp compiles csrc/navset_host.cpp (with
csrc/navfield_host.cpp, the tile counts' home) -- the offsets rule with every refusal, the field index per goal, the sizes and
launch shapes at the test shapes and at 4096 x 4096 x 65535 without overflow, the report's workgroup count, the refusals of
gather and paths -- under -fsanitize=address,undefined into a program of its own, with no HIP header on its include path.
The C++ mirror's set compiles and what needs no device runs.  Host code only: no GPU needed, and nothing is loaded into
Python."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")


def test_navset_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_navset")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_navset.cpp"),
                           os.path.join(CSRC, "navset_host.cpp"), os.path.join(CSRC, "navfield_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout


def test_cpp_mirror_compiles_and_its_refusals_run(tmp_path):
    """lom::NavFieldSet and lom::NavField::adopt of the C++ mirror compile with plain g++; without an argument the program only
    runs the refusals that come before any device is looked at (tests/test_navset_gpu.py runs the rest)."""
    exe = str(tmp_path / "test_navset_mirror")
    libdir = os.path.join(ROOT, "lidar_odometry_demo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_navset_mirror.cpp"), "-o", exe, "-L", libdir,
                           "-llidar_odometry_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
