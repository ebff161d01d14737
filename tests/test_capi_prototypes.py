"""The ctypes prototypes of lidar_odometry_demo_amd/capi.py against include/lidar_odometry_amd.h: every `ret lom_name(params)`
declaration of the header has its argtypes set, as many as the declaration has top-level parameters, and the restype its
return type maps to.  The three functions the header declares through function typedefs are given explicitly.  A function
ctypes knows nothing about takes a Python int as a 32-bit C int and returns a 32-bit int: a handle passed or a pointer
returned that way is cut in half.  Needs the built library and no device."""
import ctypes as C
import os
import re

from tests.conftest import ROOT

RESTYPE = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "double": C.c_double,
           "void": None, "void *": C.c_void_p, "const char *": C.c_char_p}
# declared as `lom_..._fn lom_name;`: (return type, parameters)
BY_TYPEDEF = {"lom_graph_pose_rotation_matrix": ("int", 2), "lom_archive_add_points": ("int64_t", 4),
              "lom_archive_add_points_device": ("int64_t", 5)}


def restype_of(ret):
    ret = re.sub(r"\s*\*\s*", " *", " ".join(ret.split()))
    if re.fullmatch(r"(const )?lom_\w+ \*", ret):
        return C.c_void_p
    return RESTYPE[ret]


def count_params(params):
    """Top-level parameters: (void) is none, and the commas within a function-pointer parameter's own parentheses are its."""
    if params.strip() in ("", "void"):
        return 0
    depth = n = 0
    for ch in params:
        depth += (ch == "(") - (ch == ")")
        n += ch == "," and depth == 0
    return n + 1


def declarations():
    """{name: (return type, number of parameters)} of every function the header declares with its parameters."""
    hdr = open(os.path.join(ROOT, "include", "lidar_odometry_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
    out = {}
    for m in re.finditer(r"\b(lom_[a-z0-9_]+)\s*\(", hdr):
        start = max(hdr.rfind(c, 0, m.start()) for c in ";{}") + 1
        ret = hdr[start:m.start()].strip()
        depth, end = 1, m.end()
        while depth:
            depth += (hdr[end] == "(") - (hdr[end] == ")")
            end += 1
        assert hdr[end:].lstrip().startswith(";"), m.group(1)
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = (ret, count_params(hdr[m.end():end - 1]))
    return out


def test_count_params():
    assert count_params("void") == 0 and count_params(" lom_map *m ") == 1
    assert count_params("lom_map *m, void (*fn)(void *user, int why), void *user") == 3


def test_prototypes_match_the_header(lom):
    L = lom.capi.lib()
    declared = declarations()
    assert len(declared) >= len(lom.capi.EXPORTED), (len(declared), len(lom.capi.EXPORTED))  # the parse lost nothing
    assert set(declared) == set(lom.capi.EXPORTED)
    assert set(BY_TYPEDEF) == set(lom.capi.EXPORTED_BY_TYPE + lom.capi.EXPORTED_BY_TYPE_POINTS)
    findings = []
    for name, (ret, n) in sorted({**declared, **BY_TYPEDEF}.items()):
        fn, wrong = getattr(L, name), []
        if fn.argtypes is None and n:  # ctypes' "not set"; for a (void) function that is as good as the empty list
            wrong.append(f"no argtypes for {n} parameters")
        elif len(fn.argtypes or ()) != n:
            wrong.append(f"{len(fn.argtypes)} argtypes for {n} parameters")
        if fn.restype is not restype_of(ret):
            wrong.append(f"restype {getattr(fn.restype, '__name__', fn.restype)} for `{ret}`")
        if wrong:
            findings.append(f"{name}: " + ", ".join(wrong))
    assert not findings, f"{len(findings)} functions:\n" + "\n".join(findings)
