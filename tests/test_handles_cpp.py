"""The handle-owning classes of the C++ mirror (include/lidar_odometry_amd.hpp): tests/cpp/test_handles_mirror.cpp, compiled
by plain g++ with -Wall -Wextra.  At compile time: none of the eleven can be copied.  Without a device: every constructor
throws the status its family's create returns and the text lom_<family>_last_error(NULL) gives -- lom::FrontEnd the literal
it has always thrown -- which is also what the same create says through ctypes.  With a device (marked gpu): create at the
smallest size, geometry and cell count, clear, one refusal per class that reaches no kernel, destroy."""
import ctypes as C

import pytest

from tests import cpp_program

CLASSES = ["FrontEnd", "PlaceDatabase", "PoseGraph", "ScanArchive", "OccupancyGrid", "ElevationGrid", "ClearanceGrid", "NavField",
           "RegionGrid", "VisibilityGrid", "RolloutGrid"]


def creates(capi):
    """(class, status, text) of every family's create through ctypes, with the arguments the program's constructors pass on"""
    L, h = capi.lib(), C.c_void_p()
    geo, egeo = capi.OccupancyGeometry(0.5, -1.0, 2.0, 3, 2), capi.ElevationGeometry(0.5, -1.0, 2.0, 3, 2, 0.25)
    out = [("FrontEnd", L.lom_frontend_create(0, None, C.byref(h)), "lom_frontend_create")]
    for name, stem, args in [("PlaceDatabase", "place_db", (C.byref(capi.PlaceParams(1, 1, 1.0, 0.0)), 0, 0)), ("PoseGraph", "graph", (0, 0, 0)),
                             ("ScanArchive", "archive", (0, 0, 0)), ("OccupancyGrid", "occupancy", (C.byref(geo), 0)),
                             ("ElevationGrid", "elevation", (C.byref(egeo), 0)), ("ClearanceGrid", "clearance", (C.byref(geo), 0)),
                             ("NavField", "navfield", (C.byref(geo), 0)), ("RegionGrid", "regions", (C.byref(geo), 0)),
                             ("VisibilityGrid", "visibility", (C.byref(geo), 0)), ("RolloutGrid", "rollout", (C.byref(geo), 0))]:
        rc = getattr(L, f"lom_{stem}_create")(*args, C.byref(h))
        out.append((name, rc, getattr(L, f"lom_{stem}_last_error")(None).decode()))
    assert h.value is None
    return out


def test_constructors_throw_what_create_says(tmp_path, lom):
    exe = cpp_program.build_with_library(tmp_path, "test_handles_mirror.cpp", ["-Werror"])  # the static_asserts: no class can be copied
    if lom.capi.lib().lom_device_count() > 0:
        pytest.skip("a GPU is visible; the refused creates are for CPU-only hosts")
    lines = cpp_program.run(exe, timeout=120).rstrip("\n").split("\n")[:-1]
    want = creates(lom.capi)
    assert [name for name, _, _ in want] == CLASSES
    assert lines == [f"{name} {rc} {text}" for name, rc, text in want]
    assert all(rc == lom.capi.ERR_NO_DEVICE for _, rc, _ in want)


@pytest.mark.gpu
def test_every_class_on_the_device(tmp_path, lom):
    exe = cpp_program.build_with_library(tmp_path, "test_handles_mirror.cpp", ["-Werror"])
    lines = cpp_program.run(exe, "device", timeout=120).rstrip("\n").split("\n")[:-1]
    assert [line.split(" ")[:2] for line in lines] == [[name, str(lom.capi.ERR_ARG)] for name in CLASSES]
    texts = dict(line.split(" ", 2)[::2] for line in lines if line.count(" ") > 1)
    assert texts["OccupancyGrid"] == "unknown occupancy option" and texts["RolloutGrid"] == "unknown rollout grid option"
