"""The visibility grid's host planning under sanitizers: tests/cpp/test_visibility.cpp compiles csrc/visibility_host.cpp --
value checks, the direction table, window sizes, launch shapes, the selection key's bit budget -- under
-fsanitize=address,undefined into a program of its own, with no HIP header on its include path.  Host code only: no GPU
needed, and nothing is loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_visibility.cpp")


def test_visibility_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_visibility")
    csrc = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, SRC, os.path.join(csrc, "visibility_host.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout
