"""The host plan of the navigation field's shift with a re-solve under sanitizers: tests/cpp/test_navfield_shift.cpp compiles
csrc/navfield_host.cpp and csrc/clearance_host.cpp under -fsanitize=address,undefined into a program of its own, with no HIP
header on its include path, and runs it directly: the clamped shift, the kept box, the entered rectangles, the trailing-border
tiles and the upload rows against brute-force counts for every side from 1 to 40 and every shift from -(n + 1) to n + 1.
Host code only: no GPU needed, nothing loaded into Python."""
import os
import re
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_navfield_shift.cpp")


def test_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_navfield_shift")
    csrc = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, SRC, os.path.join(csrc, "navfield_host.cpp"),
                           os.path.join(csrc, "clearance_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert int(re.search(r"plans: (\d+)", r.stdout).group(1)) > 80000
