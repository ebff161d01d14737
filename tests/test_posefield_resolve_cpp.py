"""The host planning of the pose field's re-solve under sanitizers: tests/cpp/test_posefield_resolve.cpp compiles
csrc/posefield_host.cpp (with csrc/navfield_host.cpp and csrc/visibility_host.cpp, as tests/test_posefield_cpp.py does) and
checks posefield::relayer_boxes -- the eight boxes k_pose_relayer runs over -- against a brute-force dilation, under
-fsanitize=address,undefined in a program of its own with no HIP header on its include path.  The C++ mirror's three
re-solve methods compile and the refusals that need no device run.  Host code only: no GPU needed, and nothing is loaded into
Python."""
from tests import cpp_program


def test_relayer_boxes_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_posefield_resolve.cpp", ["posefield_host.cpp", "navfield_host.cpp", "visibility_host.cpp"])
    cpp_program.run(exe, timeout=300)


def test_cpp_mirror_compiles_and_its_refusals_run(tmp_path):
    exe = cpp_program.build_with_library(tmp_path, "test_posefield_resolve_mirror.cpp")
    cpp_program.run(exe, timeout=120)
