"""The host planner of the elevation grid under sanitizers: tests/cpp/test_elevation.cpp with -DELEVATION_HOST_STANDALONE
compiles csrc/elevation_host.cpp and csrc/assemble_host.cpp themselves under -fsanitize=address,undefined into a program of
its own -- every value range, the origins' start cells and range verdict, every refusal of the planner in the definition's
order, launches under a cap, empty scans and an empty call.  Host code only: no GPU needed, and nothing is loaded into
Python."""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_elevation.cpp")


def test_elevation_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_elevation_host")
    csrc = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DELEVATION_HOST_STANDALONE", "-I", os.path.join(ROOT, "include"),
                           "-I", csrc, SRC, os.path.join(csrc, "elevation_host.cpp"), os.path.join(csrc, "assemble_host.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout
