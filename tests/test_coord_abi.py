"""The coordinate-block entry points (SSCN) load and validate their arguments on
the host, before any HIP call: no GPU needed."""
import ctypes

import numpy as np

COORD = ("krcn_coord_gradient", "krcn_coord_hessian", "krcn_coord_update", "krcn_csr_set_coord_window")


def test_symbols_and_signatures():
    from krcn import _lib
    lib = _lib.load()
    for name in COORD:
        assert hasattr(lib, name), f"libkrcn.so does not export {name}"
        assert name in _lib.SIGNATURES
    assert _lib.KRCN_COORD_MAX == 1024


def test_null_handle_is_invalid_before_any_hip_call():
    from krcn import _lib
    lib = _lib.load()
    cols = np.array([0, 1], dtype=np.int32)
    cp = cols.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(4)
    op = out.ctypes.data_as(_lib._dp)
    assert lib.krcn_coord_gradient(None, 2, cp, None, None, None, 0.0, op, None) == _lib.KRCN_ERR_INVALID
    assert b"null handle" in lib.krcn_last_error_string()
    assert lib.krcn_coord_hessian(None, 2, cp, None, 0.0, op, None) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_coord_update(None, 2, cp, op, None, None, None) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_csr_set_coord_window(None, 64) == _lib.KRCN_ERR_INVALID
