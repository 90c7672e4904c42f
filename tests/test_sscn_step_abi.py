"""The device SSCN step's C ABI without a GPU: include/krcn.h declares
krcn_cubic_dense, krcn_sscn_step and KRCN_SSCN_MAX, krcn/_lib.py mirrors them,
the library exports the symbols, argument validation comes before any HIP
call, and SSCN accepts device_step.  The dense-subproblem fixture
(tests/golden/f10_cubic_dense.npz) is pinned to the CPU oracle, bitwise."""
import ctypes
import inspect
import os
import re

import numpy as np
import numpy.linalg as la
import pytest

from conftest import REPO, load_golden

HEADER = os.path.join(REPO, "include", "krcn.h")


def header_text():
    return open(HEADER).read()


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_calls_and_the_limit():
    from krcn import _lib
    text = strip_comments(header_text())
    assert re.search(r"krcn_status\s+krcn_cubic_dense\s*\(", text)
    assert re.search(r"krcn_status\s+krcn_sscn_step\s*\(", text)
    m = re.search(r"KRCN_SSCN_MAX\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.KRCN_SSCN_MAX == 128
    # the header's habit: each call cites the reference lines it replaces
    raw = header_text()
    assert "cubic.py:40-75" in raw and "cubic.py:352-398" in raw


def count_params(name):
    text = strip_comments(header_text())
    args = re.search(name + r"\s*\(([^)]*)\)", text).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_signatures_match_the_header():
    from krcn import _lib
    for name in ("krcn_cubic_dense", "krcn_sscn_step"):
        assert name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name]) == count_params(name)
        assert _lib.SIGNATURES[name][-2] == ctypes.POINTER(_lib.CrnInfo)
        assert _lib.SIGNATURES[name][-1] == ctypes.c_void_p
    assert len(_lib.SIGNATURES["krcn_cubic_dense"]) == 11
    assert len(_lib.SIGNATURES["krcn_sscn_step"]) == 18


def test_library_exports_the_symbols():
    from krcn import _lib
    lib = _lib.load()
    assert hasattr(lib, "krcn_cubic_dense") and hasattr(lib, "krcn_sscn_step")


def test_null_handle_calls_are_invalid():
    from krcn import _lib
    lib = _lib.load()
    info = _lib.CrnInfo()
    H = (ctypes.c_double * 4)(1.0, 0.1, 0.1, 1.0)
    g = (ctypes.c_double * 2)(0.3, -0.2)
    s = (ctypes.c_double * 2)()
    st = lib.krcn_cubic_dense(None, 2, H, g, 1e-3, 0.1, 1e-8, 100, s, ctypes.byref(info), None)
    assert st == _lib.KRCN_ERR_INVALID
    assert b"krcn_cubic_dense" in lib.krcn_last_error_string()
    cols = (ctypes.c_int32 * 2)(0, 1)
    st = lib.krcn_sscn_step(None, 2, cols, None, None, None, 0.0, 0.0, 1e-3, 0.5, 0.1, 1e-8, 100, 20, None, None,
                            ctypes.byref(info), None)
    assert st == _lib.KRCN_ERR_INVALID
    assert b"krcn_sscn_step" in lib.krcn_last_error_string()


class _Loss:
    """What Optimizer.__init__ and SSCN.__init__ read of a loss."""
    shard = None
    hessian_lipschitz = 1.0


def test_sscn_accepts_device_step_and_refuses_a_block_above_the_limit():
    from krcn import _lib
    from optimizer.cubic import SSCN
    assert inspect.signature(SSCN.__init__).parameters["device_step"].default is False
    opt = SSCN(loss=_Loss(), reg_coef=1e-3, subspace_dim=_lib.KRCN_SSCN_MAX, tqdm=False, device_step=True)
    assert opt.device_step is True
    assert SSCN(loss=_Loss(), reg_coef=1e-3, subspace_dim=129, tqdm=False).device_step is False
    with pytest.raises(ValueError, match="subspace_dim"):
        SSCN(loss=_Loss(), reg_coef=1e-3, subspace_dim=129, tqdm=False, device_step=True)


def test_dense_fixture_is_the_oracles_output_bitwise():
    """Every case of f10_cubic_dense.npz against oracle.krcn_oracle.cubic_solver_root
    (the reference's scipy / numpy calls): s, iterations, lam and the model
    decrease bitwise; the indefinite case raises."""
    import warnings

    import krcn_oracle as O
    f = load_golden("f10_cubic_dense.npz")
    n = len(f["hidx"])
    assert n == 65 and sorted(set(f["group"])) == [0, 1, 2]
    for c in range(n):
        h = int(f["hidx"][c])
        H, g = f[f"H_{h}"], f[f"g_{h}"]
        args = (g, H, float(f["M"][c]))
        kw = dict(epsilon=float(f["eps"][c]), r0=float(f["r0"][c]))
        if f["raises"][c]:
            assert f["group"][c] == 2
            with pytest.raises(la.LinAlgError), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                O.cubic_solver_root(*args, **kw)
            continue
        s, its, lam, dec = O.cubic_solver_root(*args, **kw)
        np.testing.assert_array_equal(s, f[f"s_{c}"])
        assert its == f["its"][c] and lam == f["lam"][c] and dec == f["dec"][c]
        if f["group"][c] == 1:
            assert 1e2 < f["cond"][c] < 1e6
