"""The odometry's host side as a program of its own: tests/cpp/test_host_stages.cpp with csrc/host_stages.cpp and csrc/host_threads.cpp, compiled
by plain g++, not loaded into Python, no GPU call.  Built twice: under -fsanitize=address,undefined it runs the four host
stages (csrc/host_stages.cpp) through worker pools of 2, 3 and 16 threads against the serial run on prefixes of frame 0
of the synth sequence (equal as bytes; the serial results are pinned to the oracle by tests/test_pipeline.py) and the
table of decode_stage_words (csrc/stage_words.hpp); under -fsanitize=thread it drives Pool and Deferred
(csrc/host_threads.hpp) on their spinning and parked paths, where no report is the pass condition."""
import os
import subprocess

import numpy as np
import pytest

from lidar_odometry_demo_amd import synth
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "test_host_stages.cpp"), os.path.join(CSRC, "host_stages.cpp"),
       os.path.join(CSRC, "host_threads.cpp")]


def _build(tmp_path, name, sanitize):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           *sanitize, "-I", CSRC, *SRC, "-o", exe, "-pthread"])
    return exe


def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout
    return r


def test_pooled_stages_and_stage_word_decoder_under_asan_ubsan(tmp_path):
    frame = synth.make_sequence_frame(0)
    assert frame.dtype.itemsize == 32 and len(frame) == 26579 and len(np.unique(frame["ring"])) == 16
    path = str(tmp_path / "frame0.bin")
    frame.tofile(path)
    exe = _build(tmp_path, "test_host_stages_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _run([exe, "stages", path])


def test_pool_and_deferred_under_tsan(tmp_path):
    exe = _build(tmp_path, "test_host_stages_tsan", ["-fsanitize=thread"])
    r = _run([exe, "threads"], env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66"))
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
