"""The odometry's host side as a program of its own: tests/cpp/test_host_stages.cpp with csrc/host_stages.cpp and csrc/host_threads.cpp, compiled
by plain g++, not loaded into Python, no GPU call.  Built twice: under -fsanitize=address,undefined it runs the four host
stages (csrc/host_stages.cpp) through worker pools of 2, 3 and 16 threads against the serial run on prefixes of frame 0
of the synth sequence (equal as bytes; the serial results are pinned to the oracle by tests/test_pipeline.py) and the
table of decode_stage_words (csrc/stage_words.hpp); under -fsanitize=thread it drives Pool and Deferred
(csrc/host_threads.hpp) on their spinning and parked paths, where no report is the pass condition."""
import os

import numpy as np

from lidar_odometry_demo_amd import synth
from tests import cpp_program

CSRC_FILES = ["host_stages.cpp", "host_threads.cpp"]
FLAGS = ["-ffp-contract=off", "-Wno-unused-parameter", "-pthread"]


def test_pooled_stages_and_stage_word_decoder_under_asan_ubsan(tmp_path):
    frame = synth.make_sequence_frame(0)
    assert frame.dtype.itemsize == 32 and len(frame) == 26579 and len(np.unique(frame["ring"])) == 16
    path = str(tmp_path / "frame0.bin")
    frame.tofile(path)
    exe = cpp_program.build_host(tmp_path, "test_host_stages.cpp", CSRC_FILES, FLAGS)
    cpp_program.run(exe, "stages", path, timeout=600)


def test_pool_and_deferred_under_tsan(tmp_path):
    exe = cpp_program.build_host(tmp_path, "test_host_stages.cpp", CSRC_FILES, FLAGS, ["-fsanitize=thread"])
    cpp_program.run(exe, "threads", timeout=600, stderr_without="ThreadSanitizer",
                    env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66"))
