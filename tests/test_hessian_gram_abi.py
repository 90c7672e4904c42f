"""krcn_hessian_gram's C ABI without a GPU: include/krcn.h declares the three
calls, krcn/_lib.py mirrors them, the library exports the symbols, argument
validation comes before any HIP call, krcn_gram_geometry answers on the CPU,
and the Python layer refuses the combinations that make no sense."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "krcn.h")
NAMES = {"krcn_hessian_gram": 5, "krcn_csr_set_gram_split": 2, "krcn_gram_geometry": 4}


def header_text():
    return open(HEADER).read()


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def count_params(name):
    args = re.search(name + r"\s*\(([^)]*)\)", strip_comments(header_text())).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_header_declares_the_calls():
    text = strip_comments(header_text())
    for name in NAMES:
        assert re.search(r"krcn_status\s+" + name + r"\s*\(", text), name
    # the header's habit: the call cites the reference lines it replaces, in the comment before it
    before = header_text().split("krcn_status krcn_hessian_gram(")[0]
    comment = re.sub(r"\s*\n \*\s*", " ", before[before.rindex("/*"):])
    assert "loss.py:249-255" in comment
    for word in ("symmetric", "split order", "krcn_csr_owned_bytes", "krcn_csr_set_pass_format"):
        assert word in comment, word


def test_lib_mirrors_the_header():
    from krcn import _lib
    for name, count in NAMES.items():
        assert len(_lib.SIGNATURES[name]) == count_params(name) == count, name
    assert _lib.SIGNATURES["krcn_hessian_gram"][2] == ctypes.c_double
    assert _lib.SIGNATURES["krcn_gram_geometry"][-1] == ctypes.POINTER(ctypes.c_int64)


def test_library_exports_the_symbols():
    from krcn import _lib
    for name in NAMES:
        assert hasattr(_lib.load(), name), name


def test_argument_errors_are_invalid_without_a_gpu():
    from krcn import _lib
    lib = _lib.load()
    some = (ctypes.c_double * 4)()          # a non-null host address: never dereferenced before the checks end
    p = ctypes.cast(some, ctypes.c_void_p)
    for args, word in (((None, p, 0.0, p, None), b"null handle"),
                       ((None, None, 0.0, p, None), b"null w"),
                       ((None, p, 0.0, None, None), b"null H")):
        assert lib.krcn_hessian_gram(*args) == _lib.KRCN_ERR_INVALID
        msg = lib.krcn_last_error_string()
        assert b"krcn_hessian_gram" in msg and word in msg, msg
    assert lib.krcn_csr_set_gram_split(None, 0) == _lib.KRCN_ERR_INVALID
    assert b"null handle" in lib.krcn_last_error_string()
    for split in (-1, 257):                 # the scalar is checked before the handle is looked at
        assert lib.krcn_csr_set_gram_split(None, split) == _lib.KRCN_ERR_INVALID
        assert b"split must be" in lib.krcn_last_error_string()
    out = (ctypes.c_int64 * 8)()
    for split in (-1, 257):
        assert lib.krcn_gram_geometry(100, 100, split, out) == _lib.KRCN_ERR_INVALID
        assert b"split" in lib.krcn_last_error_string()
    assert lib.krcn_gram_geometry(100, 100, 0, None) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_gram_geometry(-1, 100, 0, out) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_gram_geometry((1 << 20) + 1, 100, 0, out) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_gram_geometry(100, -1, 0, out) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_gram_geometry(100, 1 << 31, 0, out) == _lib.KRCN_ERR_INVALID


def test_gram_geometry_answers_on_the_cpu():
    import krcn
    g = krcn.gram_geometry(5000, 6000)
    T, KS = g["T"], g["KS"]
    nt = -(-5000 // T)
    assert g == dict(T=T, KS=KS, nt=nt, tiles=nt * (nt + 1) // 2, slabs=-(-6000 // KS), split=1,
                     grid=nt * (nt + 1) // 2, ws_bytes=0)
    # a forced split is taken as it is, and its partials are counted
    g = krcn.gram_geometry(T + 1, 3 * KS + 2, split=7)
    assert (g["nt"], g["tiles"], g["slabs"], g["split"], g["grid"]) == (2, 3, 4, 7, 21)
    assert g["ws_bytes"] == 21 * T * T * 8
    # few tiles and many slabs: the rule splits, towards one workgroup per CU
    g = krcn.gram_geometry(1100, 50_000)
    assert g["tiles"] < 256 <= g["tiles"] * g["split"] and g["tiles"] * (g["split"] - 1) < 256
    # few tiles and few slabs: no split
    assert krcn.gram_geometry(40, 48)["split"] == 1
    assert krcn.gram_geometry(0, 0) == dict(T=T, KS=KS, nt=0, tiles=0, slabs=0, split=1, grid=0, ws_bytes=0)


class _NoDevice:
    """A loss that must not be touched: the argument check comes first."""
    shard = None
    l2 = 0.0

    def __getattr__(self, name):
        raise AssertionError(f"hessian looked at {name} before refusing its arguments")


def test_hessian_rejects_gram_with_block():
    from optimizer.loss import LogisticRegression
    p = inspect.signature(LogisticRegression.hessian).parameters
    assert list(p) == ["self", "x", "block", "gram"]
    assert p["block"].default is None and p["gram"].default is False
    with pytest.raises(ValueError, match="gram=True"):
        LogisticRegression.hessian(_NoDevice(), np.zeros(3), block=4, gram=True)


class _Loss:
    """What Optimizer.__init__ and Cubic_LS.__init__ read of a loss."""
    shard = None
    hessian_lipschitz = 1.0


def test_cubic_ls_gram_hessian_needs_full():
    from optimizer.cubic import Cubic_LS
    assert inspect.signature(Cubic_LS.__init__).parameters["gram_hessian"].default is False
    assert Cubic_LS(loss=_Loss(), reg_coef=1e-3, tqdm=False).gram_hessian is False
    opt = Cubic_LS(loss=_Loss(), reg_coef=1e-3, cubic_solver="full", tqdm=False, gram_hessian=True)
    assert opt.gram_hessian is True and opt.cubic_solver == opt.cubic_solver_root_full
    with pytest.raises(ValueError, match="CG"):
        Cubic_LS(loss=_Loss(), reg_coef=1e-3, cubic_solver="CG", tqdm=False, gram_hessian=True)
    with pytest.raises(ValueError, match="gram_hessian"):
        Cubic_LS(loss=_Loss(), reg_coef=1e-3, tqdm=False, gram_hessian=True)   # the default solver is "CG"


def test_device_csr_has_the_methods():
    from krcn.device import DeviceCSR
    p = inspect.signature(DeviceCSR.hessian_gram).parameters
    assert list(p) == ["self", "w", "l2", "out"] and p["l2"].default == 0.0 and p["out"].default is None
    assert list(inspect.signature(DeviceCSR.set_gram_split).parameters) == ["self", "split"]
