"""The pose field's move rule and host planning under sanitizers: tests/cpp/test_posefield.cpp compiles csrc/pose_rule.hpp
and csrc/posefield_host.cpp (with csrc/navfield_host.cpp, the rule of the cell-cost parameters, and csrc/visibility_host.cpp,
the direction table's home) -- the headings, the six moves with their conditions and weights, every refusal of the parameter
and footprint checks, the stencils, the launch shapes up to 8192 x 8192 -- under -fsanitize=address,undefined into a program
of its own, with no HIP header on its include path.  The C++ mirror's PoseField compiles and what needs no device runs.
Host code only: no GPU needed, and nothing is loaded into Python."""
from tests import cpp_program


def test_posefield_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_posefield.cpp", ["posefield_host.cpp", "navfield_host.cpp", "visibility_host.cpp"])
    cpp_program.run(exe, timeout=300)


def test_cpp_mirror_compiles_and_its_refusals_run(tmp_path):
    """lom::PoseField of the C++ mirror compiles with plain g++; without an argument the program only runs the refusals that
    come before any device is looked at and the host-only helpers (tests/test_posefield_gpu.py runs the rest)."""
    exe = cpp_program.build_with_library(tmp_path, "test_posefield_mirror.cpp")
    cpp_program.run(exe, timeout=120)
