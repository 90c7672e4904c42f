"""The batched Krylov-CRN entry points (krcn_gradient_block / krcn_value_block /
krcn_cubic_tridiag_block / krcn_crn_step_block) load and validate their
arguments on the host, before any HIP call: no GPU needed.  The scalar ranges
are checked before the handle is looked at, so their messages can be read here
without one."""
import ctypes

NAMES = {"krcn_gradient_block": 9, "krcn_value_block": 9, "krcn_cubic_tridiag_block": 14, "krcn_crn_step_block": 24}


def test_symbols_and_signatures():
    from krcn import _lib
    lib = _lib.load()
    for name, nargs in NAMES.items():
        assert hasattr(lib, name), f"libkrcn.so does not export {name}"
        assert len(_lib.SIGNATURES[name]) == nargs
    assert _lib.SIGNATURES["krcn_crn_step_block"][22] == ctypes.POINTER(_lib.CrnInfo)
    assert _lib.SIGNATURES["krcn_cubic_tridiag_block"][12] == ctypes.POINTER(_lib.CrnInfo)


def test_python_layer_has_the_methods():
    from krcn.device import DeviceCSR
    from optimizer import cubic
    for name in ("gradient_block", "value_block", "cubic_tridiag_block", "crn_step_block"):
        assert callable(getattr(DeviceCSR, name))
    assert callable(cubic.Cubic_Krylov_LS_Batch)
    assert callable(cubic.Cubic_Krylov_LS_Batch.run)


def gradient(lib, k=2, b_cols=1):
    return lib.krcn_gradient_block(None, k, None, None, b_cols, None, None, None, None)


def value(lib, k=2, b_cols=1):
    return lib.krcn_value_block(None, k, None, None, b_cols, None, None, None, None)


def tridiag(lib, k=2, m=3, it_max=100):
    return lib.krcn_cubic_tridiag_block(None, k, m, None, None, None, None, None, None, 1e-8, it_max, None, None, None)


def step(lib, k=2, b_cols=1, m=3, ls_beta=0.5, solver_it_max=100, max_trials=20):
    return lib.krcn_crn_step_block(None, k, None, None, b_cols, None, None, None, m, 1e-6, None, None, ls_beta, None,
                                   1e-8, solver_it_max, max_trials, None, None, None, None, None, None, None)


CALLS = {"krcn_gradient_block": gradient, "krcn_value_block": value, "krcn_cubic_tridiag_block": tridiag,
         "krcn_crn_step_block": step}


def invalid(lib, fn, message, **kw):
    from krcn import _lib
    assert CALLS[fn](lib, **kw) == _lib.KRCN_ERR_INVALID, (fn, kw)
    err = lib.krcn_last_error_string()
    assert f"{fn}: {message}".encode() in err, (fn, kw, err)


def test_null_handle_is_invalid_before_any_hip_call():
    from krcn import _lib
    lib = _lib.load()
    for fn in CALLS:
        invalid(lib, fn, "null handle")


def test_k_range():
    from krcn import _lib
    lib = _lib.load()
    for fn in CALLS:
        for k in (0, -1, _lib.KRCN_BLOCK_MAX + 1):
            invalid(lib, fn, f"k = {k} outside [1, 16]", k=k)
        for k in (1, _lib.KRCN_BLOCK_MAX):   # in range: the next check answers
            invalid(lib, fn, "null handle", k=k)


def test_m_range():
    from krcn import _lib
    lib = _lib.load()
    for fn in ("krcn_cubic_tridiag_block", "krcn_crn_step_block"):
        for m in (0, -3, 2045):
            invalid(lib, fn, f"m = {m} outside [1, 2044]", m=m)
        for m in (1, 2044):
            invalid(lib, fn, "null handle", m=m)


def test_b_cols():
    from krcn import _lib
    lib = _lib.load()
    for fn in ("krcn_gradient_block", "krcn_value_block", "krcn_crn_step_block"):
        for k, b_cols in ((4, 2), (4, 0), (1, 2), (16, 15)):
            invalid(lib, fn, f"b_cols = {b_cols} is neither 1 nor k = {k}", k=k, b_cols=b_cols)
        for k, b_cols in ((4, 4), (4, 1), (1, 1)):
            invalid(lib, fn, "null handle", k=k, b_cols=b_cols)


def test_line_search_and_solver_ranges():
    from krcn import _lib
    lib = _lib.load()
    fn = "krcn_crn_step_block"
    invalid(lib, fn, "max_trials must be >= 0", max_trials=-1)
    invalid(lib, fn, "null handle", max_trials=0)
    for ls_beta in (0.0, 1.0, -0.5, 1.5, float("nan")):
        invalid(lib, fn, "ls_beta must lie in (0, 1)", ls_beta=ls_beta)
    for ls_beta in (1e-3, 0.999):
        invalid(lib, fn, "null handle", ls_beta=ls_beta)
    invalid(lib, fn, "solver_it_max must be >= 1", solver_it_max=0)
    invalid(lib, fn, "null handle", solver_it_max=1)
    invalid(lib, "krcn_cubic_tridiag_block", "it_max must be >= 1", it_max=0)
    invalid(lib, "krcn_cubic_tridiag_block", "null handle", it_max=1)
