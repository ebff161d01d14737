"""The handle core shared by every device handle (csrc/device_handle.hpp): tests/cpp/test_device_handle.cpp is compiled
by plain g++ under -fsanitize=address,undefined into a program of its own and run.  It checks the size rule of the
grow-only buffers, move / swap / release of empty DeviceBuf / PinnedBuf and the texts of fail / create_fail.  The header
names hipFree, hipHostFree and hipGetErrorString, so the program links the HIP runtime; it makes no call that needs a
device."""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_device_handle.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_device_handle_core_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_device_handle")
    csrc = os.path.join(ROOT, "lidar_odometry_demo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"),
                           "-I", csrc, SRC, "-o", exe, "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
                           f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout
