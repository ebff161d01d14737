"""The pose field's move rule and host planning under sanitizers: tests/cpp/test_posefield.cpp compiles csrc/pose_rule.hpp
and csrc/posefield_host.cpp (with csrc/navfield_host.cpp, the rule of the cell-cost parameters, and csrc/visibility_host.cpp,
the direction table's home) -- the headings, the six moves with their conditions and weights, every refusal of the parameter
and footprint checks, the stencils, the launch shapes up to 8192 x 8192 -- under -fsanitize=address,undefined into a program
of its own, with no HIP header on its include path.  The C++ mirror's PoseField compiles and what needs no device runs.
Host code only: no GPU needed, and nothing is loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")


def test_posefield_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_posefield")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_posefield.cpp"),
                           os.path.join(CSRC, "posefield_host.cpp"), os.path.join(CSRC, "navfield_host.cpp"),
                           os.path.join(CSRC, "visibility_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout


def test_cpp_mirror_compiles_and_its_refusals_run(tmp_path):
    """lom::PoseField of the C++ mirror compiles with plain g++; without an argument the program only runs the refusals that
    come before any device is looked at and the host-only helpers (tests/test_posefield_gpu.py runs the rest)."""
    exe = str(tmp_path / "test_posefield_mirror")
    libdir = os.path.join(ROOT, "lidar_odometry_demo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_posefield_mirror.cpp"), "-o", exe, "-L", libdir,
                           "-llidar_odometry_amd", "-pthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
