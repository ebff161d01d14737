"""The C++ side of the scan archive and the map assembly: tests/cpp/test_assemble.cpp is compiled twice by plain g++.
Against the library it checks the mirror lom::ScanArchive / VoxelGrid::assemble (include/lidar_odometry_amd.hpp) and the
host function; with -DASSEMBLE_HOST_STANDALONE it compiles csrc/assemble_host.cpp itself under
-fsanitize=address,undefined into a program of its own and runs the planner on degenerate and extreme inputs.  Host code
only: no GPU needed (with one, the first program also assembles a small map)."""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_assemble.cpp")


def test_cpp_mirror_assemble(tmp_path, lom):
    exe = str(tmp_path / "test_assemble")
    libdir = os.path.join(ROOT, "lidar_odometry_demo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-llidar_odometry_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ALL PASSED" in r.stdout


def test_assemble_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_assemble_host")
    csrc = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DASSEMBLE_HOST_STANDALONE", "-I", os.path.join(ROOT, "include"),
                           "-I", csrc, SRC, os.path.join(csrc, "assemble_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout
