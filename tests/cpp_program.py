"""The one place that compiles and runs the suite's C++ programs (tests/cpp/*.cpp, each a stand-alone executable with its
own main that ends in check.hpp's closing line).  Two builders, one per shape a program has, and one runner; whatever a
program needs beyond its shape -- a -D, -Werror, -pthread, another include path -- is passed at the call site."""
import os
import subprocess

from tests.conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "lidar_odometry_demo_amd")
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def _compile(tmp_path, source, flags, more=()):
    """source is a file of tests/cpp, or an absolute path; the executable takes its name"""
    exe = str(tmp_path / os.path.splitext(os.path.basename(source))[0])
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, os.path.join(CPP, source), *more, "-o", exe])
    return exe


def build_host(tmp_path, source, csrc=(), flags=(), sanitize=SANITIZE):
    """Host code as a program of its own: source with the named files of csrc/, no HIP header on the include path, under
    the sanitizers unless told otherwise (sanitize=() for none)."""
    return _compile(tmp_path, source, ["-g", "-Wall", "-Wextra", *sanitize, *flags, "-I", CSRC], [os.path.join(CSRC, f) for f in csrc])


def build_with_library(tmp_path, source, flags=()):
    """A program against include/ and the built library"""
    return _compile(tmp_path, source, ["-Wall", "-Wextra", *flags, "-I", INCLUDE],
                    ["-L", LIBDIR, "-llidar_odometry_amd", "-pthread", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])


def run(exe, *args, timeout, env=None, stderr_without=None):
    """Exit status 0 and ALL PASSED, or the tail of both streams; returns stdout for what else a call site asserts"""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout, env=env)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, tail
    assert stderr_without is None or stderr_without not in r.stderr, tail
    return r.stdout
