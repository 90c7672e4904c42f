"""The tridiagonal route of the device SSCN step without a GPU: include/krcn.h
declares krcn_dense_tridiag_geometry, krcn_dense_tridiag,
krcn_cubic_dense_tridiag, krcn_sscn_step_tridiag and KRCN_SSCN_TRIDIAG_MAX,
krcn/_lib.py mirrors them, the library exports the symbols, argument validation
comes before any HIP call, the geometry is host arithmetic, and the Python
layer keeps the Cholesky route's cap and refuses subproblem="tridiag" without
device_step.  The k = 129 fixture
(tests/golden/f11_cubic_dense_tridiag.npz) is pinned to the CPU oracle, bitwise."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden

HEADER = os.path.join(REPO, "include", "krcn.h")
CALLS = ("krcn_dense_tridiag_geometry", "krcn_dense_tridiag", "krcn_cubic_dense_tridiag", "krcn_sscn_step_tridiag")


def header_text():
    return open(HEADER).read()


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def count_params(name):
    args = re.search(name + r"\s*\(([^)]*)\)", strip_comments(header_text())).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_header_declares_the_calls_and_the_limit():
    from krcn import _lib
    text = strip_comments(header_text())
    for name in CALLS:
        assert re.search(r"krcn_status\s+" + name + r"\s*\(", text), name
    m = re.search(r"KRCN_SSCN_TRIDIAG_MAX\s*=\s*(\d+)", text)
    c = re.search(r"KRCN_COORD_MAX\s*=\s*(\d+)", text)
    assert m and c and int(m.group(1)) == int(c.group(1)) == 1024
    assert _lib.KRCN_SSCN_TRIDIAG_MAX == _lib.KRCN_COORD_MAX == 1024
    assert _lib.KRCN_SSCN_MAX == 128   # the Cholesky route keeps its cap


def test_signatures_match_the_header():
    from krcn import _lib
    for name in CALLS:
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == count_params(name), name
    # the two solver calls have the signatures of the calls they extend
    assert _lib.SIGNATURES["krcn_cubic_dense_tridiag"] == _lib.SIGNATURES["krcn_cubic_dense"]
    assert _lib.SIGNATURES["krcn_sscn_step_tridiag"] == _lib.SIGNATURES["krcn_sscn_step"]
    assert len(_lib.SIGNATURES["krcn_dense_tridiag"]) == 8
    assert len(_lib.SIGNATURES["krcn_dense_tridiag_geometry"]) == 3


def test_library_exports_the_symbols():
    from krcn import _lib
    lib = _lib.load()
    for name in CALLS:
        assert hasattr(lib, name), name


def _solver_args(k=2):
    H = (ctypes.c_double * max(k * k, 1))(*([0.0] * max(k * k, 1)))
    g = (ctypes.c_double * max(k, 1))()
    s = (ctypes.c_double * max(k, 1))()
    return H, g, s


def test_argument_errors_come_before_any_hip_call():
    """No GPU here: a call that reached the HIP runtime would return KRCN_ERR_HIP
    (or fault on the fake handle), so KRCN_ERR_INVALID shows the order."""
    from krcn import _lib
    lib = _lib.load()
    info = _lib.CrnInfo()
    H, g, s = _solver_args()
    al, be = (ctypes.c_double * 2)(), (ctypes.c_double * 2)()
    buf = ctypes.create_string_buffer(1 << 16)
    fake = ctypes.c_void_p(ctypes.addressof(buf))   # a non-null handle: these checks come before it is read
    inv = _lib.KRCN_ERR_INVALID
    # null handle
    assert lib.krcn_dense_tridiag(None, 2, H, g, al, be, None, None) == inv
    assert b"krcn_dense_tridiag" in lib.krcn_last_error_string()
    assert lib.krcn_cubic_dense_tridiag(None, 2, H, g, 1e-3, 0.1, 1e-8, 100, s, ctypes.byref(info), None) == inv
    assert b"krcn_cubic_dense_tridiag" in lib.krcn_last_error_string()
    cols = (ctypes.c_int32 * 2)(0, 1)
    assert lib.krcn_sscn_step_tridiag(None, 2, cols, None, None, None, 0.0, 0.0, 1e-3, 0.5, 0.1, 1e-8, 100, 20, None,
                                      None, ctypes.byref(info), None) == inv
    assert b"krcn_sscn_step_tridiag" in lib.krcn_last_error_string()
    # k = 0 and k = 1025 (the handle is looked at for nullness alone before k)
    for k in (0, 1025):
        assert lib.krcn_dense_tridiag(fake, k, H, g, al, be, None, None) == inv
        assert f"k = {k}".encode() in lib.krcn_last_error_string()
        assert lib.krcn_cubic_dense_tridiag(fake, k, H, g, 1e-3, 0.1, 1e-8, 100, s, ctypes.byref(info), None) == inv
        assert f"k = {k}".encode() in lib.krcn_last_error_string()
    # null pointers
    for args in ((None, g, al, be), (H, None, al, be), (H, g, None, be), (H, g, al, None)):
        assert lib.krcn_dense_tridiag(fake, 2, *args, None, None) == inv
    for args in ((None, g, s, ctypes.byref(info)), (H, None, s, ctypes.byref(info)), (H, g, None, ctypes.byref(info)),
                 (H, g, s, None)):
        assert lib.krcn_cubic_dense_tridiag(fake, 2, args[0], args[1], 1e-3, 0.1, 1e-8, 100, args[2], args[3],
                                            None) == inv
    # it_max < 1
    assert lib.krcn_cubic_dense_tridiag(fake, 2, H, g, 1e-3, 0.1, 1e-8, 0, s, ctypes.byref(info), None) == inv
    assert b"it_max" in lib.krcn_last_error_string()


def geometry(k):
    from krcn import _lib
    lib = _lib.load()
    launches, ws = ctypes.c_int64(-1), ctypes.c_int64(-1)
    st = lib.krcn_dense_tridiag_geometry(k, ctypes.byref(launches), ctypes.byref(ws))
    return st, launches.value, ws.value


def ws_bytes(k):
    """B and the reflector rows (K = k + 1 rows of ld doubles each, ld = K rounded
    up to a 64-byte line), then nine rows: two p, tau, alphas, betas, g, s_T and
    two for the selection's 3 k int32."""
    K = k + 1
    ld = (K + 7) // 8 * 8
    return 8 * ld * (2 * K + 9)


def test_geometry_is_host_arithmetic():
    from krcn import _lib
    assert geometry(1) == (0, 0, 832) and ws_bytes(1) == 832
    assert geometry(2) == (0, 1, 960) and ws_bytes(2) == 960
    assert geometry(1024) == (0, 1023, 16_999_104) and ws_bytes(1024) == 16_999_104
    for k in (3, 63, 64, 65, 128, 129, 500, 1000):
        assert geometry(k) == (0, k - 1, ws_bytes(k)), k
    for k in (0, -1, 1025):
        assert geometry(k)[0] == _lib.KRCN_ERR_INVALID
    lib = _lib.load()
    v = ctypes.c_int64(0)
    assert lib.krcn_dense_tridiag_geometry(4, None, ctypes.byref(v)) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_dense_tridiag_geometry(4, ctypes.byref(v), None) == _lib.KRCN_ERR_INVALID
    import krcn
    assert krcn.DeviceCSR.dense_tridiag_geometry(1024) == (1023, 16_999_104)


class _Loss:
    """What Optimizer.__init__ and SSCN.__init__ read of a loss."""
    shard = None
    hessian_lipschitz = 1.0


def test_sscn_subproblem_argument():
    from optimizer.cubic import SSCN
    assert inspect.signature(SSCN.__init__).parameters["subproblem"].default == "cholesky"
    mk = lambda **kw: SSCN(loss=_Loss(), reg_coef=1e-3, tqdm=False, **kw)   # noqa: E731
    for k in (1, 129, 500, 1024):
        opt = mk(subspace_dim=k, device_step=True, subproblem="tridiag")
        assert opt.device_step is True and opt.subproblem == "tridiag"
    for k in (0, 1025):
        with pytest.raises(ValueError, match="subspace_dim"):
            mk(subspace_dim=k, device_step=True, subproblem="tridiag")
    # the default subproblem keeps the present refusal above 128
    assert mk(subspace_dim=128, device_step=True).subproblem == "cholesky"
    with pytest.raises(ValueError, match="subspace_dim"):
        mk(subspace_dim=129, device_step=True)
    with pytest.raises(ValueError, match="subspace_dim"):
        mk(subspace_dim=129, device_step=True, subproblem="cholesky")
    # the tridiagonal route is the device step's alone
    with pytest.raises(ValueError, match="device_step"):
        mk(subspace_dim=10, subproblem="tridiag")
    with pytest.raises(ValueError, match="subproblem"):
        mk(subspace_dim=10, device_step=True, subproblem="lanczos")


def test_device_csr_has_the_calls_with_the_default_route():
    import krcn
    p = inspect.signature(krcn.DeviceCSR.sscn_step).parameters
    assert p["subproblem"].default == "cholesky"
    assert inspect.signature(krcn.DeviceCSR.dense_tridiag).parameters["want_q"].default is False
    assert "M" in inspect.signature(krcn.DeviceCSR.cubic_dense_tridiag).parameters


def test_k129_fixture_is_the_oracles_output_bitwise():
    """Every case of f11_cubic_dense_tridiag.npz against
    oracle.krcn_oracle.cubic_solver_root (the reference's scipy / numpy calls)."""
    import krcn_oracle as O
    f = load_golden("f11_cubic_dense_tridiag.npz")
    n = len(f["hidx"])
    assert n == 8 and sorted(set(f["group"])) == [0, 1] and not f["raises"].any()
    assert sorted(set(f["M"])) == [1e-3, 1.0] and sorted(set(f["eps"])) == [float(np.finfo(float).eps), 1e-8]
    for c in range(n):
        h = int(f["hidx"][c])
        H, g = f[f"H_{h}"], f[f"g_{h}"]
        assert H.shape == (129, 129) and g.shape == (129,)
        s, its, lam, dec = O.cubic_solver_root(g, H, float(f["M"][c]), epsilon=float(f["eps"][c]),
                                               r0=float(f["r0"][c]))
        np.testing.assert_array_equal(s, f[f"s_{c}"])
        assert its == f["its"][c] and lam == f["lam"][c] and dec == f["dec"][c]
        if f["group"][c] == 1:
            assert 1e2 < f["cond"][c] < 1e6
    largest = max(os.path.getsize(os.path.join(REPO, "tests", "golden", n)) for n in os.listdir(
        os.path.join(REPO, "tests", "golden")) if n.endswith(".npz") and not n.startswith("f11"))
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "f11_cubic_dense_tridiag.npz")) <= largest
