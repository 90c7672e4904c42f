"""The device Krylov-CRN step's C ABI without a GPU: include/krcn.h declares
krcn_cubic_tridiag, krcn_crn_step and krcn_crn_info, krcn/_lib.py mirrors them,
the library exports the symbols, and argument validation comes before any HIP
call."""
import ctypes
import os
import re

from conftest import REPO

HEADER = os.path.join(REPO, "include", "krcn.h")

# the C types of krcn_crn_info's members, by ctypes type
C_TYPES = {"int": ctypes.c_int, "double": ctypes.c_double}


def header_text():
    return open(HEADER).read()


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_step_calls_and_the_record():
    text = strip_comments(header_text())
    assert re.search(r"krcn_status\s+krcn_cubic_tridiag\s*\(", text)
    assert re.search(r"krcn_status\s+krcn_crn_step\s*\(", text)
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*krcn_crn_info\s*;", text)
    # the header's habit: each call cites the reference lines it replaces
    raw = header_text()
    assert "cubic.py:40-75" in raw and "cubic.py:265-309" in raw


def test_struct_layout_matches_the_header():
    from krcn import _lib
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*krcn_crn_info\s*;", strip_comments(header_text())).group(1)
    members = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    want = [(name, _lib.LanczosInfo if ctype == "krcn_lanczos_info" else C_TYPES[ctype]) for ctype, name in members]
    assert [(n, t) for n, t in _lib.CrnInfo._fields_] == want
    assert [n for n, _ in want] == ["accepted", "trials", "solver_it", "solver_status", "reg_coef", "lam",
                                    "model_decrease", "value_new", "dx_norm", "lanczos"]
    # 4 ints, 5 doubles, then krcn_lanczos_info (4 ints, 2 doubles): no padding anywhere
    assert ctypes.sizeof(_lib.CrnInfo) == 16 + 40 + ctypes.sizeof(_lib.LanczosInfo) == 88
    assert _lib.CrnInfo.reg_coef.offset == 16 and _lib.CrnInfo.lanczos.offset == 56


def count_params(name):
    text = strip_comments(header_text())
    args = re.search(name + r"\s*\(([^)]*)\)", text).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_signatures_match_the_header():
    from krcn import _lib
    for name in ("krcn_cubic_tridiag", "krcn_crn_step"):
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name]) == count_params(name)
    sig = _lib.SIGNATURES["krcn_crn_step"]
    assert sig[-2] == ctypes.POINTER(_lib.CrnInfo) and sig[-1] == ctypes.c_void_p
    assert _lib.SIGNATURES["krcn_cubic_tridiag"][-2] == ctypes.POINTER(_lib.CrnInfo)


def test_library_exports_the_symbols():
    from krcn import _lib
    lib = _lib.load()
    assert hasattr(lib, "krcn_cubic_tridiag") and hasattr(lib, "krcn_crn_step")


def test_null_handle_calls_are_invalid():
    from krcn import _lib
    lib = _lib.load()
    info = _lib.CrnInfo()
    al = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    be = (ctypes.c_double * 2)(0.1, 0.1)
    s = (ctypes.c_double * 3)()
    st = lib.krcn_cubic_tridiag(None, 3, al, be, 1.0, 1e-3, 0.1, 1e-8, 100, s, ctypes.byref(info), None)
    assert st == _lib.KRCN_ERR_INVALID
    assert b"krcn_cubic_tridiag" in lib.krcn_last_error_string()
    st = lib.krcn_crn_step(None, None, None, None, 0.0, 10, 0, 1e-6, 0.0, 1e-3, 0.5, 0.1, 1e-8, 100, 20, None, None,
                           None, None, None, ctypes.byref(info), None)
    assert st == _lib.KRCN_ERR_INVALID
    assert b"krcn_crn_step" in lib.krcn_last_error_string()
