"""The handle core shared by every device handle (csrc/device_handle.hpp): tests/cpp/test_device_handle.cpp is compiled
by plain g++ under -fsanitize=address,undefined into a program of its own and run.  It checks the size rule of the
grow-only buffers, move / swap / release of empty DeviceBuf / PinnedBuf and the texts of fail / create_fail.  The header
names hipFree, hipHostFree and hipGetErrorString, so the program links the HIP runtime; it makes no call that needs a
device."""
import os

from tests import cpp_program

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_device_handle_core_under_sanitizers(tmp_path):
    # the one program with the HIP runtime's headers and library: neither builder's shape, so the flags stand here
    exe = cpp_program.build_host(tmp_path, "test_device_handle.cpp", [],
                                 ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"), "-L", os.path.join(ROCM, "lib"),
                                  "-lamdhip64", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"])
    cpp_program.run(exe, timeout=300)
