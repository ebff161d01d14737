"""The matcher's launch planning under sanitizers: tests/cpp/test_match_plan.cpp compiles csrc/match_plan.cpp -- the grids
and k_lm shapes of a scan, the rounds of the batched align and of the batched quality report, the block offsets inside a
round's buffers -- under -fsanitize=address,undefined into a program of its own, with no HIP header on its include path.
Host code only: no GPU needed, and nothing is loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_match_plan.cpp")


def test_match_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_match_plan")
    csrc = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", csrc, SRC, os.path.join(csrc, "match_plan.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout
    # the figures the comment at kQualBatchBudgetBytes (csrc/match_plan.hpp) quotes
    assert "holds 47 problems of 28,800 points or 708 of 1,900" in r.stdout
