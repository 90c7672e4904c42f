"""krcn_cgs2 loads and validates its arguments on the host, before any HIP
call: no GPU needed.  The range of k is checked before the handle is looked
at, so its message can be read here without one."""
import ctypes


def cgs2(lib, h=None, k=3):
    return lib.krcn_cgs2(h, k, None, None, None, None, None)


def test_symbol_and_signature():
    from krcn import _lib
    lib = _lib.load()
    assert hasattr(lib, "krcn_cgs2"), "libkrcn.so does not export krcn_cgs2"
    sig = _lib.SIGNATURES["krcn_cgs2"]
    assert len(sig) == 7
    assert sig[1] == ctypes.c_int
    assert sig[4] == ctypes.POINTER(ctypes.c_double) and sig[5] == ctypes.POINTER(ctypes.c_int)
    assert lib.krcn_cgs2.argtypes == sig


def test_python_layer_has_the_method():
    from krcn.device import DeviceCSR
    assert callable(DeviceCSR.cgs2)


def test_null_handle_is_invalid_before_any_hip_call():
    from krcn import _lib
    lib = _lib.load()
    assert cgs2(lib) == _lib.KRCN_ERR_INVALID
    assert b"krcn_cgs2: null handle" in lib.krcn_last_error_string()


def test_k_range():
    from krcn import _lib
    lib = _lib.load()
    for k in (0, -1, 2044, 2048, 1 << 30):
        assert cgs2(lib, k=k) == _lib.KRCN_ERR_INVALID
        assert f"krcn_cgs2: k = {k} outside [1, 2043]".encode() in lib.krcn_last_error_string()
    for k in (1, 2043):   # in range: the next check answers
        assert cgs2(lib, k=k) == _lib.KRCN_ERR_INVALID
        assert b"krcn_cgs2: null handle" in lib.krcn_last_error_string()
