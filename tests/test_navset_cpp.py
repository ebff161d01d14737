"""The navigation field set's host planning under sanitizers: tests/cpp/test_navset.cpp compiles csrc/navset_host.cpp (with
csrc/navfield_host.cpp, the tile counts' home) -- the offsets rule with every refusal, the field index per goal, the sizes and
launch shapes at the test shapes and at 4096 x 4096 x 65535 without overflow, the report's workgroup count, the refusals of
gather and paths -- under -fsanitize=address,undefined into a program of its own, with no HIP header on its include path.
The C++ mirror's set compiles and what needs no device runs.  Host code only: no GPU needed, and nothing is loaded into
Python."""
from tests import cpp_program


def test_navset_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_navset.cpp", ["navset_host.cpp", "navfield_host.cpp"])
    cpp_program.run(exe, timeout=300)


def test_cpp_mirror_compiles_and_its_refusals_run(tmp_path):
    """lom::NavFieldSet and lom::NavField::adopt of the C++ mirror compile with plain g++; without an argument the program only
    runs the refusals that come before any device is looked at (tests/test_navset_gpu.py runs the rest)."""
    exe = cpp_program.build_with_library(tmp_path, "test_navset_mirror.cpp")
    cpp_program.run(exe, timeout=120)
