"""The host planner of the scan votes under sanitizers: tests/cpp/test_vote.cpp with -DVOTE_HOST_STANDALONE compiles
csrc/vote_host.cpp and csrc/assemble_host.cpp themselves under -fsanitize=address,undefined into a program of its own --
refusals, the slices of 1, 63, 64, 65 and 129 scans, descriptor offsets, the origin's verdict, the step bound.  Host code
only: no GPU needed, and nothing is loaded into Python."""
from tests import cpp_program


def test_vote_host_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_vote.cpp", ["vote_host.cpp", "assemble_host.cpp"],
                                 ["-DVOTE_HOST_STANDALONE", "-I", cpp_program.INCLUDE])
    cpp_program.run(exe, timeout=300)
