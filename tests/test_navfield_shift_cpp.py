"""The host plan of the navigation field's shift with a re-solve under sanitizers: tests/cpp/test_navfield_shift.cpp compiles
csrc/navfield_host.cpp and csrc/clearance_host.cpp under -fsanitize=address,undefined into a program of its own, with no HIP
header on its include path, and runs it directly: the clamped shift, the kept box, the entered rectangles, the trailing-border
tiles and the upload rows against brute-force counts for every side from 1 to 40 and every shift from -(n + 1) to n + 1.
Host code only: no GPU needed, nothing loaded into Python."""
import re

from tests import cpp_program


def test_plan_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_navfield_shift.cpp", ["navfield_host.cpp", "clearance_host.cpp"])
    stdout = cpp_program.run(exe, timeout=300)
    assert int(re.search(r"plans: (\d+)", stdout).group(1)) > 80000
