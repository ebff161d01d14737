"""tests/cpp_program.py and tests/cpp/check.hpp on a program of six lines: one passing CHECK goes through the host builder and
the runner; the same program with a failing CHECK makes the runner raise, and what it shows names the file and the line.
Host code only: a failed CHECK is a line of output and an exit status, not a fault."""
import pytest

from tests import cpp_program

PROGRAM = """#include "check.hpp"
int main()
{
    CHECK(%s);
    return check_done();
}
"""


def build(tmp_path, condition):
    source = tmp_path / "six_lines.cpp"
    source.write_text(PROGRAM % condition)
    return cpp_program.build_host(tmp_path, str(source), flags=["-I", cpp_program.CPP])


def test_a_passing_check_passes(tmp_path):
    assert cpp_program.run(build(tmp_path, "1 + 1 == 2"), timeout=60) == "ALL PASSED\n"


def test_a_failing_check_raises_with_file_and_line(tmp_path):
    exe = build(tmp_path, "1 == 2")
    with pytest.raises(AssertionError) as failure:
        cpp_program.run(exe, timeout=60)
    assert f"FAILED {tmp_path / 'six_lines.cpp'}:4: 1 == 2\nFAILED (1)\n" in str(failure.value)
