"""The cut of a call's scans into launches under sanitizers: tests/cpp/test_launch_cut.cpp compiles csrc/assemble_host.cpp
(the cutter) and the three planners that use it -- csrc/vote_host.cpp, csrc/occupancy_host.cpp, csrc/elevation_host.cpp --
under -fsanitize=address,undefined into a program of its own.  Host code only: no GPU needed, and nothing is loaded into
Python."""
from tests import cpp_program


def test_launch_cut_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_launch_cut.cpp", [f + "_host.cpp" for f in ("assemble", "vote", "occupancy", "elevation")],
                                 ["-I", cpp_program.INCLUDE])
    cpp_program.run(exe, timeout=300)
