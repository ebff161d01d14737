"""The per-point arithmetic of the evaluation (csrc/k_eval.hpp: point_terms, huber_terms) as a program of its own:
tests/cpp/test_point_terms.cpp, compiled by hipcc (the header is HIP; the functions under test are __host__ __device__ and
run here on the host), not loaded into Python, no GPU call.  It holds the closed-form rotation columns and the Huber terms
without square root and divide to the forms they replace, both measured against a long double evaluation of the
reference's formulas: the new form's worst error may be at most twice the old form's.  Built plain and once with the
host side under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

from tests import cpp_program
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_point_terms.cpp")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("sanitize", [[], SANITIZE], ids=["plain", "asan_ubsan"])
def test_point_terms_new_forms_against_old(tmp_path, sanitize):
    exe = str(tmp_path / "test_point_terms")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Wno-unused-parameter", *sanitize, "-I", CSRC, SRC, "-o", exe])
    print(cpp_program.run(exe, timeout=300))
