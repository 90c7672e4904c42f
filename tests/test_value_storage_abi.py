"""The value-storage policy's ABI surface (krcn_csr_set_value_storage,
krcn_csr_plan_value_bytes) and the golden problem of its GPU tests:
tests/golden/f9_dense_values32.npz is f8's problem with every matrix value
rounded to fp32 and widened back (make_golden_dense_values32.py).  No GPU
needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import krcn_oracle as O
from conftest import REPO, golden_csr, load_golden

HEADER = os.path.join(REPO, "include", "krcn.h")
NAMES = {"KRCN_VALUES_FULL": 0, "KRCN_VALUES_F32": 1, "KRCN_VALUES_F32_EXACT": 2}
FUNCS = ("krcn_csr_set_value_storage", "krcn_csr_plan_value_bytes")


@pytest.fixture(scope="module")
def f8():
    return load_golden("f8_dense.npz")


@pytest.fixture(scope="module")
def f9():
    return load_golden("f9_dense_values32.npz")


def test_header_declares_the_policy():
    text = open(HEADER).read()
    for name, value in NAMES.items():
        assert re.search(rf"\b{name}\s*=\s*{value}\b", text), name
    assert re.search(r"krcn_status\s+krcn_csr_set_value_storage\s*\(\s*krcn_csr\s*\*\s*h\s*,\s*int\s+values\s*\)", text)
    assert re.search(r"krcn_status\s+krcn_csr_plan_value_bytes\s*\(\s*krcn_csr\s*\*\s*h\s*,\s*int\s*\*\s*out2_host\s*\)",
                     text)


def test_binding_matches_the_header():
    from krcn import _lib
    text = open(HEADER).read()
    for name in NAMES:
        assert getattr(_lib, name) == int(re.search(rf"\b{name}\s*=\s*(\d+)", text).group(1))
    assert _lib.SIGNATURES["krcn_csr_set_value_storage"] == [ctypes.c_void_p, ctypes.c_int]
    assert _lib.SIGNATURES["krcn_csr_plan_value_bytes"] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]


def test_library_exports_both_symbols():
    from krcn import _lib
    lib = _lib.load()
    for fn in FUNCS:
        assert hasattr(lib, fn), fn


def test_null_arguments_are_invalid():
    from krcn import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 2)()
    assert lib.krcn_csr_set_value_storage(None, _lib.KRCN_VALUES_F32) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_csr_plan_value_bytes(None, out) == _lib.KRCN_ERR_INVALID
    # (a null output with a live handle needs a device: tests/test_gpu_value_storage.py)
    assert lib.krcn_csr_plan_value_bytes(None, None) == _lib.KRCN_ERR_INVALID


def test_f9_is_f8_with_fp32_values(f8, f9):
    for key in ("shape", "indptr", "indices", "b", "b01", "x", "v0", "v1", "v2", "l2s"):
        np.testing.assert_array_equal(f9[key], f8[key], err_msg=key)
    np.testing.assert_array_equal(f9["data"], f8["data"].astype(np.float32).astype(np.float64))
    assert not np.any(f9["data"] == f8["data"])   # no value of f8 is fp32-exact
    assert set(f9.keys()) == set(f8.keys())


def test_oracle_reproduces_f9_bitwise(f9):
    A = golden_csr(f9)
    b01 = O.labels01(f9["b"])
    x = f9["x"]
    np.testing.assert_array_equal(b01, f9["b01"])
    for t, l2 in enumerate(f9["l2s"]):
        np.testing.assert_array_equal(O.mat_vec_product(A, x), f9[f"Ax_l2_{t}"])
        assert O.value(A, b01, x, l2=l2) == f9[f"value_l2_{t}"]
        np.testing.assert_array_equal(O.gradient(A, b01, x, l2=l2), f9[f"grad_l2_{t}"])
        for k in range(3):
            np.testing.assert_array_equal(O.hess_vec_prod(A, x, f9[f"v{k}"], l2=l2), f9[f"hvp{k}_l2_{t}"])
    g = O.gradient(A, b01, x)
    np.testing.assert_array_equal(g, f9["g"])
    w = O.hessian_weights(A, x)
    for m in (10, 20):
        V, al, be, beta = O.lanczos(lambda v: O.hvp_from_weights(A, w, v), g, m)
        np.testing.assert_array_equal(al, f9[f"alphas_m{m}"])
        np.testing.assert_array_equal(be, f9[f"betas_m{m}"])
        np.testing.assert_array_equal(V, f9[f"V_m{m}"])
        assert beta == f9[f"beta_m{m}"]


def test_f9_differs_from_f8_where_the_tests_tell_them_apart(f8, f9):
    """The GPU tests hold a narrowed pass to f9 at 1e-13 and ask that it miss f8 by more than
    1e-10: the two references must be that far apart."""
    from conftest import rel_err
    for k in range(3):
        assert rel_err(f9[f"hvp{k}_l2_0"], f8[f"hvp{k}_l2_0"]) > 1e-9
    assert rel_err(f9["Ax_l2_0"], f8["Ax_l2_0"]) > 1e-9
