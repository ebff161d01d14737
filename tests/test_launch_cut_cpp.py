"""The cut of a call's scans into launches under sanitizers: tests/cpp/test_launch_cut.cpp compiles csrc/assemble_host.cpp
(the cutter) and the three planners that use it -- csrc/vote_host.cpp, csrc/occupancy_host.cpp, csrc/elevation_host.cpp --
under -fsanitize=address,undefined into a program of its own.  Host code only: no GPU needed, and nothing is loaded into
Python."""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_launch_cut.cpp")


def test_launch_cut_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_launch_cut")
    csrc = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc, SRC] +
                          [os.path.join(csrc, f + "_host.cpp") for f in ("assemble", "vote", "occupancy", "elevation")] +
                          ["-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout
