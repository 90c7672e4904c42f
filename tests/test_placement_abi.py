"""The placement override's ABI surface (krcn_csr_set_placement_keep and its
getter).  No GPU needed: the range of `keep` is checked before the handle is
touched, so both refusals can be told apart by their messages here; what the
override does to a live handle is tests/test_gpu_placement.py."""
import ctypes
import os
import re

from conftest import REPO

HEADER = os.path.join(REPO, "include", "krcn.h")
FUNCS = ("krcn_csr_set_placement_keep", "krcn_csr_get_placement_keep")


def test_header_declares_the_override():
    text = open(HEADER).read()
    assert re.search(r"krcn_status\s+krcn_csr_set_placement_keep\s*\(\s*krcn_csr\s*\*\s*h\s*,\s*int\s+keep\s*\)", text)
    assert re.search(r"krcn_status\s+krcn_csr_get_placement_keep\s*\(\s*const\s+krcn_csr\s*\*\s*h\s*,"
                     r"\s*int\s*\*\s*keep_host\s*\)", text)
    # the usual comment: what it replaces in the reference
    comment = text[:text.index("krcn_status krcn_csr_set_placement_keep")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("Replaces no reference call. */")


def test_binding_matches_the_header():
    from krcn import _lib
    assert _lib.SIGNATURES["krcn_csr_set_placement_keep"] == [ctypes.c_void_p, ctypes.c_int]
    assert _lib.SIGNATURES["krcn_csr_get_placement_keep"] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]


def test_library_exports_both_symbols():
    from krcn import _lib
    lib = _lib.load()
    for fn in FUNCS:
        assert hasattr(lib, fn), fn


def test_null_handle_and_out_of_range_are_refused():
    from krcn import _lib
    lib = _lib.load()
    for keep in (-1, 0, 7):
        assert lib.krcn_csr_set_placement_keep(None, keep) == _lib.KRCN_ERR_INVALID
        assert b"null handle" in lib.krcn_last_error_string()
    for keep in (-2, 8, 1 << 20):
        assert lib.krcn_csr_set_placement_keep(None, keep) == _lib.KRCN_ERR_INVALID
        msg = lib.krcn_last_error_string()
        assert b"0..7" in msg and str(keep).encode() in msg and b"null" not in msg
    out = ctypes.c_int(5)
    assert lib.krcn_csr_get_placement_keep(None, ctypes.byref(out)) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_csr_get_placement_keep(None, None) == _lib.KRCN_ERR_INVALID
    assert out.value == 5
