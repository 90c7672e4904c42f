"""The batched Lanczos entry points (krcn_lanczos_block / krcn_basis_combine_block /
krcn_weights_block) load and validate their arguments on the host, before any
HIP call: no GPU needed.  The scalar ranges are checked before the handle is
looked at, so their messages can be read here without one."""
import ctypes

NAMES = ("krcn_lanczos_block", "krcn_basis_combine_block", "krcn_weights_block")


def test_symbols_and_signatures():
    from krcn import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), f"libkrcn.so does not export {name}"
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["krcn_lanczos_block"]) == 13
    assert len(_lib.SIGNATURES["krcn_basis_combine_block"]) == 8
    assert len(_lib.SIGNATURES["krcn_weights_block"]) == 5
    assert _lib.SIGNATURES["krcn_lanczos_block"][11] == ctypes.POINTER(_lib.LanczosInfo)


def test_python_layer_has_the_methods():
    from krcn.device import DeviceCSR
    from optimizer.loss import LogisticRegression
    for name in ("lanczos_block", "basis_combine_block", "weights_block"):
        assert callable(getattr(DeviceCSR, name))
    assert callable(LogisticRegression.lanczos_block)


def lanczos_block(lib, h=None, k=2, w_cols=1, m=3):
    return lib.krcn_lanczos_block(h, k, None, w_cols, None, m, 1e-6, None, None, None, None, None, None)


def test_null_handle_is_invalid_before_any_hip_call():
    from krcn import _lib
    lib = _lib.load()
    assert lanczos_block(lib) == _lib.KRCN_ERR_INVALID
    assert b"krcn_lanczos_block: null handle" in lib.krcn_last_error_string()
    assert lib.krcn_basis_combine_block(None, 2, 3, None, None, None, None, None) == _lib.KRCN_ERR_INVALID
    assert b"krcn_basis_combine_block: null handle" in lib.krcn_last_error_string()
    assert lib.krcn_weights_block(None, 2, None, None, None) == _lib.KRCN_ERR_INVALID
    assert b"krcn_weights_block: null handle" in lib.krcn_last_error_string()


def test_k_range():
    from krcn import _lib
    lib = _lib.load()
    for k in (0, -1, _lib.KRCN_BLOCK_MAX + 1):
        assert lanczos_block(lib, k=k, w_cols=k) == _lib.KRCN_ERR_INVALID
        assert f"krcn_lanczos_block: k = {k} outside [1, 16]".encode() in lib.krcn_last_error_string()
        assert lib.krcn_basis_combine_block(None, k, 3, None, None, None, None, None) == _lib.KRCN_ERR_INVALID
        assert f"k = {k} outside [1, 16]".encode() in lib.krcn_last_error_string()
        assert lib.krcn_weights_block(None, k, None, None, None) == _lib.KRCN_ERR_INVALID
        assert f"k = {k} outside [1, 16]".encode() in lib.krcn_last_error_string()
    for k in (1, _lib.KRCN_BLOCK_MAX):   # in range: the next check answers
        assert lanczos_block(lib, k=k) == _lib.KRCN_ERR_INVALID
        assert b"null handle" in lib.krcn_last_error_string()


def test_m_range():
    from krcn import _lib
    lib = _lib.load()
    for m in (0, -3, 2045):
        assert lanczos_block(lib, m=m) == _lib.KRCN_ERR_INVALID
        assert f"krcn_lanczos_block: m = {m} outside [1, 2044]".encode() in lib.krcn_last_error_string()
        assert lib.krcn_basis_combine_block(None, 2, m, None, None, None, None, None) == _lib.KRCN_ERR_INVALID
        assert f"m = {m} outside [1, 2044]".encode() in lib.krcn_last_error_string()
    for m in (1, 2044):
        assert lanczos_block(lib, m=m) == _lib.KRCN_ERR_INVALID
        assert b"null handle" in lib.krcn_last_error_string()


def test_w_cols():
    from krcn import _lib
    lib = _lib.load()
    for k, w_cols in ((4, 2), (4, 0), (1, 2), (16, 15)):
        assert lanczos_block(lib, k=k, w_cols=w_cols) == _lib.KRCN_ERR_INVALID
        assert f"w_cols = {w_cols} is neither 1 nor k = {k}".encode() in lib.krcn_last_error_string()
    for k, w_cols in ((4, 4), (4, 1), (1, 1)):
        assert lanczos_block(lib, k=k, w_cols=w_cols) == _lib.KRCN_ERR_INVALID
        assert b"null handle" in lib.krcn_last_error_string()
