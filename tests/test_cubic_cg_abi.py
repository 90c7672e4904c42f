"""krcn_cubic_cg's C ABI without a GPU: include/krcn.h declares the call and its
record, krcn/_lib.py mirrors them, the library exports the symbol, argument
validation comes before any HIP call (scalars before the handle), and Cubic_LS
accepts device_solver."""
import ctypes
import inspect
import math
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "krcn.h")


def header_text():
    return open(HEADER).read()


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_call_and_the_record():
    text = strip_comments(header_text())
    assert re.search(r"krcn_status\s+krcn_cubic_cg\s*\(", text)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*krcn_cubic_cg_info\s*;", text)
    assert m
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip()
              for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == ["solver_it", "solver_status", "cg_solves", "cg_unconverged", "cg_iterations", "ticks",
                      "reg_coef", "lam", "model_decrease", "s_norm"]
    # the header's habit: each call cites the reference lines it replaces
    assert "cubic.py:152-182" in header_text().split("krcn_cubic_cg_info;")[1].split("krcn_cubic_cg(")[0]


def count_params(name):
    text = strip_comments(header_text())
    args = re.search(name + r"\s*\(([^)]*)\)", text).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_lib_mirrors_the_header():
    from krcn import _lib
    sig = _lib.SIGNATURES["krcn_cubic_cg"]
    assert len(sig) == count_params("krcn_cubic_cg") == 13
    assert sig[-2] == ctypes.POINTER(_lib.CubicCgInfo) and sig[-1] == ctypes.c_void_p
    # 4 ints, 2 int64, 4 doubles, no padding
    assert ctypes.sizeof(_lib.CubicCgInfo) == 4 * 4 + 2 * 8 + 4 * 8 == 64
    assert [f[0] for f in _lib.CubicCgInfo._fields_] == [
        "solver_it", "solver_status", "cg_solves", "cg_unconverged", "cg_iterations", "ticks", "reg_coef", "lam",
        "model_decrease", "s_norm"]
    assert _lib.CubicCgInfo.cg_iterations.offset == 16 and _lib.CubicCgInfo.reg_coef.offset == 32


def test_library_exports_the_symbol():
    from krcn import _lib
    assert hasattr(_lib.load(), "krcn_cubic_cg")


GOOD = dict(l2=0.0, M=1e-3, r0=0.1, eps=1e-8, it_max=100, cg_rtol=1e-8, cg_maxiter=0)


def call_null(**over):
    """The call with a null handle and null vectors: only the scalars can differ."""
    from krcn import _lib
    lib = _lib.load()
    a = dict(GOOD, **over)
    info = _lib.CubicCgInfo()
    st = lib.krcn_cubic_cg(None, None, None, a["l2"], a["M"], a["r0"], a["eps"], a["it_max"], a["cg_rtol"],
                           a["cg_maxiter"], None, ctypes.byref(info), None)
    return st, lib.krcn_last_error_string()


@pytest.mark.parametrize("over,word", [
    (dict(it_max=0), b"it_max"),
    (dict(cg_rtol=-1.0), b"cg_rtol"),
    (dict(cg_rtol=math.nan), b"cg_rtol"),
    (dict(M=0.0), b"M must"),
    (dict(M=-1.0), b"M must"),
    (dict(M=math.inf), b"M must"),
    (dict(M=math.nan), b"M must"),
    (dict(eps=-1e-8), b"eps"),
    (dict(eps=math.nan), b"eps"),
    (dict(), b"null handle"),
])
def test_argument_errors_are_invalid_without_a_gpu(over, word):
    """Scalar ranges are checked before the handle is looked at, so a null
    handle tells them apart by the message; good scalars reach the handle check."""
    from krcn import _lib
    st, msg = call_null(**over)
    assert st == _lib.KRCN_ERR_INVALID
    assert b"krcn_cubic_cg" in msg and word in msg, msg


class _Loss:
    """What Optimizer.__init__ and Cubic_LS.__init__ read of a loss."""
    shard = None
    hessian_lipschitz = 1.0


class _ShardedLoss(_Loss):
    shard = "rows"


def test_cubic_ls_accepts_device_solver():
    from optimizer.cubic import Cubic_LS
    assert inspect.signature(Cubic_LS.__init__).parameters["device_solver"].default is False
    assert Cubic_LS(loss=_Loss(), reg_coef=1e-3, tqdm=False).device_solver is False
    opt = Cubic_LS(loss=_Loss(), reg_coef=1e-3, cubic_solver="CG", tqdm=False, device_solver=True)
    assert opt.device_solver is True and opt.cubic_solver == opt.cubic_solver_root_CG
    with pytest.raises(ValueError, match="full"):
        Cubic_LS(loss=_Loss(), reg_coef=1e-3, cubic_solver="full", tqdm=False, device_solver=True)
    with pytest.raises(NotImplementedError):
        Cubic_LS(loss=_ShardedLoss(), reg_coef=1e-3, tqdm=False, device_solver=True)
    # off: "full" is still accepted
    assert Cubic_LS(loss=_Loss(), reg_coef=1e-3, cubic_solver="full", tqdm=False).device_solver is False


def test_device_csr_has_cubic_cg():
    from krcn.device import DeviceCSR
    p = inspect.signature(DeviceCSR.cubic_cg).parameters
    assert list(p) == ["self", "w", "g", "M", "l2", "r0", "eps", "it_max", "cg_rtol", "cg_maxiter", "out"]
    assert p["l2"].default == 0.0 and p["r0"].default == 0.1 and p["eps"].default == 1e-8
    assert p["it_max"].default == 100 and p["cg_rtol"].default is None and p["cg_maxiter"].default is None
