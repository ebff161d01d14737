"""The matcher's launch planning under sanitizers: tests/cpp/test_match_plan.cpp compiles csrc/match_plan.cpp -- the grids
and k_lm shapes of a scan, the rounds of the batched align and of the batched quality report, the block offsets inside a
round's buffers -- under -fsanitize=address,undefined into a program of its own, with no HIP header on its include path.
Host code only: no GPU needed, and nothing is loaded into Python."""
from tests import cpp_program


def test_match_plan_under_sanitizers(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_match_plan.cpp", ["match_plan.cpp"])
    stdout = cpp_program.run(exe, timeout=300)
    # the figures the comment at kQualBatchBudgetBytes (csrc/match_plan.hpp) quotes
    assert "holds 47 problems of 28,800 points or 708 of 1,900" in stdout
