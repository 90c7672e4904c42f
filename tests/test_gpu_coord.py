"""Coordinate-block kernels of SSCN (krcn_coord_gradient / _hessian / _update)
against what the reference's partial_gradient, partial_hessian and
update_mat_vec_product returned (tests/golden/f7_coord.npz, 300 x 120 with a
dense column, an empty column and a repeated index in the selection) and
against scipy on a problem with longer columns.

Tolerances: fp64 1e-13 (what the suite holds krcn_gradient and the dense
Hessian to: the sums differ from the reference's in order only, the margin is
the device expit's), fp32 1e-5 (the suite's fp32 HVP tolerance), the update
bitwise (scipy's csc_matvec order).  Every case runs with the automatic LDS
window (one window) and with 64-row windows (five windows on n = 300; the dense
column and several others straddle the boundaries).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.special
import torch

import krcn
import krcn_oracle as O
from conftest import golden_csr, load_golden, rel_err
from krcn import _lib, synth
from optimizer.cubic import SSCN
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu
DEV = "cuda"
WINDOWS = [0, 64]


def t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def h(x):
    return x.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def f7():
    return load_golden("f7_coord.npz")


@pytest.fixture(scope="module")
def X64(f7):
    return krcn.DeviceCSR(golden_csr(f7))


@pytest.fixture(scope="module")
def X32(f7):
    return krcn.DeviceCSR(golden_csr(f7), dtype=torch.float32)


def status_of(exc):
    return exc.value.status


# ----------------------------------------------------- vs the reference fixture
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("li", [0, 1])
def test_gradient_hessian_vs_reference_fp64(f7, X64, window, li):
    X64.set_coord_window(window)
    l2 = float(f7["l2s"][li])
    Ax, b, x, I = t(f7[f"Ax_l2_{li}"]), t(f7["b01"]), t(f7["x"]), f7["I"]
    g = X64.coord_gradient(I, Ax, b, x, l2)
    H = X64.coord_hessian(I, Ax, l2)
    eg, eh = rel_err(g, f7[f"grad_l2_{li}"]), rel_err(H, f7[f"hess_l2_{li}"])
    print(f"window {window} l2 {l2}: gradient rel err {eg:.3e}, hessian rel err {eh:.3e}")
    assert g.dtype == np.float64 and g.shape == (len(I),) and H.shape == (len(I), len(I))
    assert eg < 1e-13
    assert eh < 1e-13


@pytest.mark.parametrize("window", WINDOWS)
def test_gradient_hessian_vs_reference_fp32(f7, X32, window):
    X32.set_coord_window(window)
    f32 = torch.float32
    for li in (0, 1):
        l2 = float(f7["l2s"][li])
        Ax, b, x, I = t(f7[f"Ax_l2_{li}"], f32), t(f7["b01"], f32), t(f7["x"], f32), f7["I"]
        eg = rel_err(X32.coord_gradient(I, Ax, b, x, l2), f7[f"grad_l2_{li}"])
        eh = rel_err(X32.coord_hessian(I, Ax, l2), f7[f"hess_l2_{li}"])
        print(f"fp32 window {window} l2 {l2}: gradient rel err {eg:.3e}, hessian rel err {eh:.3e}")
        assert eg < 1e-5
        assert eh < 1e-5


@pytest.mark.parametrize("window", WINDOWS)
def test_hessian_structure(f7, X64, window):
    """Exactly symmetric; positions 0 and 6 of the selection repeat column 5:
    their rows and columns carry the same bits (with l2 the reference's
    l2 * eye(k) sits on the two diagonal entries alone); position 3 is the
    empty column: l2 on the diagonal, zero elsewhere."""
    X64.set_coord_window(window)
    I = f7["I"]
    assert I[0] == I[6] and I[3] == 1
    Ax = t(f7["Ax_l2_0"])
    H0 = X64.coord_hessian(I, Ax, 0.0)
    H1 = X64.coord_hessian(I, Ax, 0.01)
    for H in (H0, H1):
        assert np.array_equal(H, H.T)
    assert np.array_equal(H0[0, :], H0[6, :]) and np.array_equal(H0[:, 0], H0[:, 6])
    rest = np.setdiff1d(np.arange(len(I)), [0, 6])
    assert np.array_equal(H1[0, rest], H1[6, rest]) and np.array_equal(H1[rest, 0], H1[rest, 6])
    assert H1[0, 0] == H1[6, 6] == H0[0, 0] + 0.01 and H1[0, 6] == H1[6, 0] == H0[0, 0]
    for H, l2 in ((H0, 0.0), (H1, 0.01)):
        row = np.zeros(len(I))
        row[3] = l2
        assert np.array_equal(H[3, :], row) and np.array_equal(H[:, 3], row)


def test_gradient_column_independence_and_k1(f7, X64):
    X64.set_coord_window(0)
    Ax, b, x, I = t(f7["Ax_l2_1"]), t(f7["b01"]), t(f7["x"]), f7["I"]
    g = X64.coord_gradient(I, Ax, b, x, 0.01)
    H = X64.coord_hessian(I, Ax, 0.01)
    for a, c in enumerate(I):
        g1 = X64.coord_gradient([c], Ax, b, x, 0.01)
        assert g1.shape == (1,) and g1[0] == g[a], f"position {a} (column {c})"
        H1 = X64.coord_hessian([c], Ax, 0.01)
        assert H1.shape == (1, 1)
        assert abs(H1[0, 0] - H[a, a]) <= 1e-13 * np.abs(H).max()


@pytest.mark.parametrize("window", WINDOWS)
def test_all_columns_and_dense_hessian(f7, window):
    A = golden_csr(f7)
    n, d = A.shape
    x = f7["x"]
    loss = LogisticRegression(A, f7["b"], l1=0, l2=0.01, store_mat_vec_prod=True)
    loss.device_matrix.set_coord_window(window)
    w = O.hessian_weights(A, x)
    ref = (A.T.multiply(w) @ A / n).toarray() + 0.01 * np.eye(d)
    H = loss.device_matrix.coord_hessian(range(d), loss._device_Ax(x), 0.01)
    e = rel_err(H, ref)
    print(f"window {window}: all-columns hessian rel err {e:.3e}")
    assert H.shape == (d, d) and e < 1e-13
    assert np.array_equal(H, H.T)
    assert np.array_equal(loss.hessian(x), H)


# ------------------------------------------------------------------- update
@pytest.mark.parametrize("window", WINDOWS)
def test_update_bitwise(f7, X64, window):
    X64.set_coord_window(window)
    A = golden_csr(f7)
    I, delta = f7["I"], f7["delta"]
    for li in (0, 1):
        Ax = t(f7[f"Ax_l2_{li}"])
        keep = Ax.clone()
        out = X64.coord_update(I, delta, Ax)
        assert out.data_ptr() != Ax.data_ptr() and torch.equal(Ax, keep)
        assert np.array_equal(h(out), f7[f"updated_l2_{li}"])
    alone = X64.coord_update(I, delta)
    assert np.array_equal(h(alone), A.tocsc()[:, I] @ delta)
    Ax = t(f7["Ax_l2_0"])
    same = X64.coord_update(I, delta, Ax, out=Ax)
    assert same.data_ptr() == Ax.data_ptr()
    assert np.array_equal(h(Ax), f7["updated_l2_0"])


def test_update_back_to_back_with_reused_host_arrays(f7, X64):
    """Two asynchronous calls in a row, the caller's cols / delta arrays
    overwritten between and after them: both see the values of their own call."""
    X64.set_coord_window(0)
    C = golden_csr(f7).tocsc()
    Ax0 = f7["Ax_l2_0"]
    Ax = t(Ax0)
    cols = np.array(f7["I"], dtype=np.int32)
    delta = np.array(f7["delta"], dtype=np.float64)
    I1, d1 = cols.copy(), delta.copy()
    I2, d2 = cols[::-1].copy(), -2.0 * delta + 0.125
    out1 = X64.coord_update(cols, delta, Ax)
    cols[:] = I2
    delta[:] = d2
    out2 = X64.coord_update(cols, delta, Ax)
    cols[:] = 0
    delta[:] = 1e9
    assert np.array_equal(h(out1), Ax0 + C[:, I1] @ d1)
    assert np.array_equal(h(out2), Ax0 + C[:, I2] @ d2)


@pytest.mark.parametrize("window", WINDOWS)
def test_determinism(f7, X64, window):
    X64.set_coord_window(window)
    Ax, b, x, I, delta = t(f7["Ax_l2_1"]), t(f7["b01"]), t(f7["x"]), f7["I"], f7["delta"]
    g, H, u = X64.coord_gradient(I, Ax, b, x, 0.01), X64.coord_hessian(I, Ax, 0.01), h(X64.coord_update(I, delta, Ax))
    for _ in range(3):
        assert np.array_equal(X64.coord_gradient(I, Ax, b, x, 0.01), g)
        assert np.array_equal(X64.coord_hessian(I, Ax, 0.01), H)
        assert np.array_equal(h(X64.coord_update(I, delta, Ax)), u)


# --------------------------------------------------------------- validation
def test_validation_without_a_launch(f7, X64):
    A = golden_csr(f7)
    d = A.shape[1]
    Ax, b = t(f7["Ax_l2_0"]), t(f7["b01"])
    for bad in ([3, -1, 4], [3, 4, d]):
        for fn in (lambda c: X64.coord_gradient(c, Ax, b), lambda c: X64.coord_hessian(c, Ax),
                   lambda c: X64.coord_update(c, np.zeros(len(c)), Ax)):
            with pytest.raises(_lib.KrcnError) as e:
                fn(bad)
            assert status_of(e) == _lib.KRCN_ERR_INVALID
            assert f"cols_host[{1 if bad[1] < 0 else 2}]" in str(e.value)
    for k in (0, _lib.KRCN_COORD_MAX + 1):
        cols = np.zeros(k, dtype=np.int32)
        for fn in (lambda c: X64.coord_gradient(c, Ax, b), lambda c: X64.coord_hessian(c, Ax),
                   lambda c: X64.coord_update(c, np.zeros(len(c)), Ax)):
            with pytest.raises(_lib.KrcnError) as e:
                fn(cols)
            assert status_of(e) == _lib.KRCN_ERR_INVALID
    with pytest.raises(_lib.KrcnError) as e:
        X64.set_coord_window(100)
    assert status_of(e) == _lib.KRCN_ERR_INVALID
    Xs = krcn.DeviceCSR(A, n_global=2 * A.shape[0], shard_mode=_lib.KRCN_SHARD_ROWS)
    for fn in (lambda: Xs.coord_gradient([0], Ax, b), lambda: Xs.coord_hessian([0], Ax),
               lambda: Xs.coord_update([0], [1.0], Ax)):
        with pytest.raises(_lib.KrcnError) as e:
            fn()
        assert status_of(e) == _lib.KRCN_ERR_UNSUPPORTED


def test_matrix_without_nonzeros():
    """n x d without nonzeros: l2 x_I, l2 I and a copy of Ax (zeros without one)."""
    A = sp.csr_matrix((5, 4), dtype=np.float64)
    X = krcn.DeviceCSR(A)
    x = np.array([0.5, -1.0, 2.0, 0.25])
    Ax, b = t(np.zeros(5)), t(np.ones(5))
    I = [2, 0, 2]
    assert np.array_equal(X.coord_gradient(I, Ax, b), np.zeros(3))
    assert np.array_equal(X.coord_gradient(I, Ax, b, t(x), 0.5), 0.5 * x[I])
    assert np.array_equal(X.coord_hessian(I, Ax, 0.5), 0.5 * np.eye(3))
    seen = t(np.arange(5.0))
    assert np.array_equal(h(X.coord_update(I, [1.0, 2.0, 3.0], seen)), np.arange(5.0))
    assert np.array_equal(h(X.coord_update(I, [1.0, 2.0, 3.0])), np.zeros(5))


def test_no_plan_build(f1):
    """Coordinate calls alone leave a fresh handle's owned bytes larger by the
    documented workspace only (cap (12 + 8 cap) device bytes, cap = k rounded
    up to a multiple of 64): no pass plans were built; a later HVP is f1's."""
    A = golden_csr(f1)
    fresh = krcn.DeviceCSR(A).owned_bytes()
    X = krcn.DeviceCSR(A)
    Ax = t(f1["Ax0"])
    b01 = t(O.labels01(f1["b"]))
    cols = np.arange(0, 100, 3)           # k = 34 -> cap 64
    X.coord_gradient(cols, Ax, b01)
    X.coord_hessian(cols, Ax)
    X.coord_update(cols, np.ones(len(cols)), Ax)
    assert X.owned_bytes() - fresh == 64 * (12 + 8 * 64)
    X.coord_hessian(np.arange(70), Ax)    # k = 70 -> cap 128: grown, the old block released
    assert X.owned_bytes() - fresh == 128 * (12 + 8 * 128)
    w = X.weights(Ax)
    assert rel_err(h(X.hvp(w, t(f1["v0"]))), f1["hvp0_0"]) < 1e-13
    assert X.owned_bytes() - fresh > 128 * (12 + 8 * 128)   # now the plans exist


# ------------------------------------------------------ through the optimizer
@pytest.mark.parametrize("li", [0, 1])
def test_loss_methods_vs_reference(f7, li):
    A = golden_csr(f7)
    l2 = float(f7["l2s"][li])
    loss = LogisticRegression(A.tocsc(), f7["b"], l1=0, l2=l2, store_mat_vec_prod=True)
    x, I = f7["x"], f7["I"]
    g = loss.partial_gradient(x, I)
    H = loss.partial_hessian(x, I)
    assert isinstance(g, np.ndarray) and g.shape == (len(I),)
    assert sp.issparse(H) and H.shape == (len(I), len(I))
    assert rel_err(g, f7[f"grad_l2_{li}"]) < 1e-13
    assert rel_err(H.toarray(), f7[f"hess_l2_{li}"]) < 1e-13
    loss.update_mat_vec_product(t(f7[f"Ax_l2_{li}"]), f7["delta"], I)
    assert loss.reuse is True and loss._w is None
    assert np.array_equal(h(loss._mat_vec_prod), f7[f"updated_l2_{li}"])


def test_sscn_runs_without_hvps(monkeypatch):
    """Six SSCN steps on the f6 problem with DeviceCSR.hvp disabled: the step
    goes through the coordinate kernels alone and follows the reference."""
    f6 = load_golden("f6_methods.npz")
    n, d, nnz = (int(v) for v in f6["shape"])
    A, b = synth.make_problem(None, seed=int(f6["seed"]), n=n, d=d, nnz=nnz)

    def no_hvp(self, *a, **kw):
        raise AssertionError("SSCN called DeviceCSR.hvp")

    monkeypatch.setattr(krcn.DeviceCSR, "hvp", no_hvp)
    loss = LogisticRegression(A.tocsc(), b, l1=0, l2=0, store_mat_vec_prod=True)
    opt = SSCN(loss=loss, reg_coef=1e-3, label="SSCN", subspace_dim=10, tolerance=1e-9, tqdm=False)
    tr = opt.run(x0=np.full(A.shape[1], 0.5), it_max=6)
    opt.compute_loss_of_iterates()
    np.testing.assert_allclose(tr.loss_vals, f6["sscn_loss_vals"], rtol=1e-10)
    assert rel_err(np.asarray(tr.xs), f6["sscn_xs"]) < 1e-10


# ------------------------------------------------------------ longer columns
@pytest.fixture(scope="module")
def longer():
    A, b = synth.make_problem(None, seed=8, n=2000, d=700, nnz=40_000)
    n = A.shape[0]
    x = np.random.default_rng(1).uniform(-0.5, 0.5, size=A.shape[1])
    I = np.random.default_rng(3).choice(700, 100, replace=False)
    delta = np.random.default_rng(4).uniform(-0.3, 0.3, size=100)
    b01 = O.labels01(b)
    Ax = A @ x
    C = A.tocsc()[:, I]
    w = O.hessian_weights(A, x)
    ref = dict(A=A, b01=b01, Ax=Ax, I=I, delta=delta,
               g=C.T @ (scipy.special.expit(Ax) - b01) / n,
               H=(C.T.multiply(w) @ C / n).toarray(), u=Ax + C @ delta)
    return ref


@pytest.mark.parametrize("window", [0, 256])
def test_longer_columns_vs_scipy(longer, window):
    X = krcn.DeviceCSR(longer["A"])
    X.set_coord_window(window)
    Ax, b = t(longer["Ax"]), t(longer["b01"])
    I = longer["I"]
    eg = rel_err(X.coord_gradient(I, Ax, b), longer["g"])
    H = X.coord_hessian(I, Ax)
    eh = rel_err(H, longer["H"])
    print(f"window {window}: gradient rel err {eg:.3e}, hessian rel err {eh:.3e}")
    assert eg < 1e-13
    assert eh < 1e-13
    assert np.array_equal(H, H.T)
    assert np.array_equal(h(X.coord_update(I, longer["delta"], Ax)), longer["u"])
