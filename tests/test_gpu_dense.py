"""The dense plan format (KRCN_FORMAT_DENSE, krcn_dense.hpp): every operation of
the library through row-major images of X and X^T.

Tolerances are the suite's: fp64 rel 1e-13 (max-norm) for Ax, weights,
gradient, loss and HVP, 1e-11 for Lanczos alphas / betas and 1e-6 for V
(test_gpu_lanczos.py), 1e-10 for the Krylov-CRN trajectory with equal
line-search decisions (test_gpu_crn.py); fp32 rel 1e-5 against the fp64
reference.  With the sequential lane policy the passes are scipy's bits.
The golden problem (tests/golden/f8_dense.npz, made by make_golden_dense.py
from the reference) is 130 x 75 at 97 % fill; m = 10 and 20 only (see there).
Every test builds the plans (plan_info) before its first compute call.
"""
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
import krcn_oracle as O
from conftest import golden_csr, load_golden, rel_err
from krcn import _lib, synth
from optimizer.cubic import Cubic_Krylov_LS
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu

DEV = "cuda"
DENSE = 5
TOL = {torch.float64: 1e-13, torch.float32: 1e-5}


def t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def h(x):
    torch.cuda.synchronize()
    return x.cpu().numpy()


def dense_handle(A, **kw):
    kw.setdefault("fmt", DENSE)
    X = krcn.DeviceCSR(A, **kw)
    X.plan_info()   # images built here, never inside a compute call
    return X


@pytest.fixture(scope="module")
def f8():
    return load_golden("f8_dense.npz")


@pytest.fixture(scope="module")
def f8_op(f8):
    """(A, dense handle, w, g) at the golden x; the handle is shared read-only."""
    A = golden_csr(f8)
    X = dense_handle(A)
    Ax = X.matvec(t(f8["x"]))
    return A, X, X.weights(Ax), X.gradient(Ax, t(f8["b01"]))


# ------------------------------------------------------------ 1. against f8
def test_objective_pieces_vs_golden(f8, f8_op):
    A, X, _, _ = f8_op
    assert X.plan_format() == {"pass1": "dense", "pass2": "dense"}
    x, b01 = t(f8["x"]), t(f8["b01"])
    Ax = X.matvec(x)
    assert rel_err(h(Ax), f8["Ax_l2_0"]) < 1e-13
    w = X.weights(Ax)
    assert rel_err(h(w), O.hessian_weights(A, f8["x"])) < 1e-13
    assert rel_err(h(X.gradient(Ax, b01)), f8["grad_l2_0"]) < 1e-13
    assert rel_err(h(X.gradient(Ax, b01, x, l2=0.01)), f8["grad_l2_1"]) < 1e-13
    assert abs(X.loss_mean(Ax, b01) - f8["value_l2_0"]) < 1e-13 * abs(f8["value_l2_0"])
    for k in range(3):
        v = t(f8[f"v{k}"])
        assert rel_err(h(X.hvp(w, v)), f8[f"hvp{k}_l2_0"]) < 1e-13
        assert rel_err(h(X.hvp(w, v, l2=0.01)), f8[f"hvp{k}_l2_1"]) < 1e-13


@pytest.mark.parametrize("m", [10, 20])
def test_lanczos_vs_golden(f8, f8_op, m):
    _, X, w, g = f8_op
    V, al, be, info = X.lanczos(w, g, m)
    assert info.m_eff == m and not info.breakdown
    assert rel_err(al, f8[f"alphas_m{m}"]) < 1e-11
    assert rel_err(be, f8[f"betas_m{m}"]) < 1e-11
    assert rel_err(h(V).T, f8[f"V_m{m}"]) < 1e-6


def test_krylov_crn_trajectory_vs_golden(f8):
    A = golden_csr(f8)
    loss = LogisticRegression(A, f8["b"], l1=0, l2=0, store_mat_vec_prod=True, format="dense")
    assert loss.device_matrix.plan_format() == {"pass1": "dense", "pass2": "dense"}
    opt = Cubic_Krylov_LS(loss=loss, reg_coef=1e-3, label="krylov", subspace_dim=10, tolerance=1e-9, tqdm=False)
    tr = opt.run(x0=np.full(A.shape[1], 0.5), it_max=8)
    opt.compute_loss_of_iterates()
    xs = np.asarray(tr.xs)
    assert xs.shape == f8["crn_xs"].shape
    assert rel_err(xs, f8["crn_xs"]) < 1e-10
    assert tr.solver_its == list(f8["crn_solver_its"])
    np.testing.assert_allclose(tr.loss_vals, f8["crn_loss_vals"], rtol=1e-10)
    assert opt.reg_coef == f8["crn_final_reg_coef"]


def test_loss_format_argument(f8):
    A = golden_csr(f8)
    with pytest.raises(ValueError):
        LogisticRegression(A, f8["b"], l1=0, l2=0, format="csr")
    wave = LogisticRegression(A, f8["b"], l1=0, l2=0, format=_lib.KRCN_FORMAT_WAVE)
    assert wave.device_matrix.plan_format() == {"pass1": "wave", "pass2": "wave"}


# -------------------------------------------- 2. the sequential policy is bitwise
def signed_zero_problem():
    A, _ = synth.make_dense_problem(67, 129, 0.9, seed=3)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(129)
    u = rng.standard_normal(67)
    v[[0, 7, 64, 128]] = [0.0, -0.0, -0.0, 0.0]
    u[[0, 33, 66]] = [-0.0, 0.0, -0.0]
    return A, u, v, rng.uniform(0.01, 0.25, 67)


def test_sequential_policy_is_bitwise_scipy(f8):
    A8 = golden_csr(f8)
    rng = np.random.default_rng(9)
    cases = [(A8, rng.standard_normal(130), f8["v0"], O.hessian_weights(A8, f8["x"])), signed_zero_problem()]
    for A, u, v, w in cases:
        X = dense_handle(A, lanes=(1, 1))
        assert X.plan_info() == {"pass1": (1, 1, -(-A.shape[0] // 256), -(-A.shape[0] // 256)),
                                 "pass2": (1, 1, -(-A.shape[1] // 256), -(-A.shape[1] // 256))}
        np.testing.assert_array_equal(h(X.matvec(t(v))), A @ v)
        np.testing.assert_array_equal(h(X.rmatvec(t(u))), (A.T @ u) / A.shape[0])
        np.testing.assert_array_equal(h(X.hvp(t(w), t(v))), O.hvp_from_weights(A, w, v))


# ----------------------------------------------------------- 3. edge shapes
def edge_matrix(n, d, nnz0=False):
    if nnz0:
        return sp.csr_matrix((n, d), dtype=np.float64)
    A, _ = synth.make_dense_problem(n, d, 0.9, seed=100 + n + d)
    return A


EDGE = [(1, 1, False), (1, 7, False), (9, 1, False), (5, 6, True), (3, 130, False), (130, 3, False),
        (67, 129, False), (300, 257, False)]


def check_passes(A, X, dtype, seed=1):
    n, d = A.shape
    rng = np.random.default_rng(seed)
    u, v, w = rng.standard_normal(n), rng.standard_normal(d), rng.uniform(0.01, 0.25, n)
    tol = TOL[dtype]
    if dtype == torch.float32:   # the fp64 reference of the values the handle holds
        A = sp.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices, A.indptr), shape=A.shape)
        u, v, w = (a.astype(np.float32).astype(np.float64) for a in (u, v, w))
    assert rel_err(h(X.matvec(t(v, dtype))), A @ v) < tol
    assert rel_err(h(X.rmatvec(t(u, dtype))), (A.T @ u) / n) < tol
    assert rel_err(h(X.hvp(t(w, dtype), t(v, dtype))), O.hvp_from_weights(A, w, v)) < tol
    assert rel_err(h(X.hvp(t(w, dtype), t(v, dtype), l2=0.01)), O.hvp_from_weights(A, w, v, 0.01)) < tol


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,d,nnz0", EDGE)
def test_edge_shapes(n, d, nnz0, dtype):
    A = edge_matrix(n, d, nnz0)
    for lanes in (0, 2, 8, 64):
        X = dense_handle(A, dtype=dtype, lanes=(lanes, lanes))
        assert X.plan_format() == {"pass1": "dense", "pass2": "dense"}
        if lanes:
            info = X.plan_info()
            assert info["pass1"][1] == lanes and info["pass2"][1] == lanes
        check_passes(A, X, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_stored_zeros_and_unsorted_columns(dtype):
    A, _ = synth.make_dense_problem(67, 129, 0.9, seed=4)
    data = A.data.copy()
    data[::5] = 0.0                         # explicit stored zeros
    Z = sp.csr_matrix((data, A.indices, A.indptr), shape=A.shape)
    assert Z.nnz == A.nnz
    idx, dat = A.indices.copy(), A.data.copy()
    for r in (0, 13, 66):                   # these rows' columns reversed
        lo, hi = A.indptr[r], A.indptr[r + 1]
        idx[lo:hi] = idx[lo:hi][::-1]
        dat[lo:hi] = dat[lo:hi][::-1]
    R = sp.csr_matrix((dat, idx, A.indptr), shape=A.shape)
    assert not np.all(np.diff(R.indices[R.indptr[13]:R.indptr[14]]) > 0)
    for M in (Z, R):
        for lanes in (0, 1):
            check_passes(M, dense_handle(M, dtype=dtype, lanes=(lanes, lanes)), dtype)


# ---------------------------------------------------------------- 4. slices
def test_forced_slices_pass1():
    """12 rows of 2,100 in 8 slices.  The Lanczos point is chosen on the CPU: H has rank 12, and
    with nearly equal weights (x within +-0.01) its 12 eigenvalues cluster so tightly that the
    oracle's own alphas move by 4e-11 when its HVP sums are reordered, so no summation order
    can hold 1e-11 there; at x within +-0.2 the weights spread over 0.004..0.16 and the same
    reorderings (six random permutations of both sums) move alphas and betas by <= 6e-15.
    m = 10 only: the recurrence breaks down at step 13."""
    A, b = synth.make_dense_problem(12, 2100, 0.95, seed=6)
    X = dense_handle(A, slicing=8)
    info = X.plan_info()
    assert info["pass1"][0] == 8 and info["pass1"][3] % 8 == 0
    check_passes(A, X, torch.float64)
    x = np.random.default_rng(2).uniform(-0.2, 0.2, 2100)
    w = O.hessian_weights(A, x)
    g = O.gradient(A, O.labels01(b), x)
    _, al, be, info = X.lanczos(t(w), t(g), 10)
    Vr, alr, ber, _ = O.lanczos(lambda q: O.hvp_from_weights(A, w, q), g, m=10)
    assert info.m_eff == 10
    assert rel_err(al, alr) < 1e-11
    assert rel_err(be, ber) < 1e-11


def test_forced_slices_pass2():
    A, _ = synth.make_dense_problem(2100, 12, 0.95, seed=7)
    X = dense_handle(A, slicing=8)
    info = X.plan_info()
    assert info["pass2"][0] == 8 and info["pass1"][0] < 8    # pass 1: 12 columns are 6 vectors
    check_passes(A, X, torch.float64)


def test_auto_slices_few_long_rows():
    A, _ = synth.make_dense_problem(12, 2100, 0.95, seed=6)
    for dtype in (torch.float64, torch.float32):
        X = dense_handle(A, dtype=dtype)
        assert X.plan_info()["pass1"][0] > 1 and X.plan_info()["pass2"][0] == 1
        check_passes(A, X, dtype)


# ----------------------------------------------------------- 5. mixed passes
@pytest.mark.parametrize("pf,names", [((5, 1), ("dense", "wave")), ((1, 5), ("wave", "dense"))])
def test_mixed_passes(f8, pf, names):
    A = golden_csr(f8)
    X = krcn.DeviceCSR(A, pass_formats=pf)
    X.plan_info()
    assert X.plan_format() == {"pass1": names[0], "pass2": names[1]}
    check_passes(A, X, torch.float64)


# ------------------------------------- 6. the rest of the library, dense plans
def test_cg_solve_matches_dense_solve(f8, f8_op):
    A, X, _, _ = f8_op
    w = O.hessian_weights(A, f8["x"])
    rhs = np.random.default_rng(2).standard_normal(A.shape[1])
    shift = 0.05
    sol, info = X.cg_solve(t(w), t(rhs), shift=shift, rtol=1e-10)
    H = (A.T.multiply(w) @ A / A.shape[0]).toarray() + shift * np.eye(A.shape[1])
    assert info.converged == 1 and info.info == 0 and 0 < info.iterations < 10 * A.shape[1]
    assert info.residual_norm < 1e-10 * np.linalg.norm(rhs)
    assert rel_err(h(sol), np.linalg.solve(H, rhs)) < 1e-8


def test_loss_values_bitwise(f8, f8_op):
    _, X, _, _ = f8_op
    b01 = t(f8["b01"])
    xs = [t(f8["x"]), t(f8["v0"] * 0.1), t(f8["crn_xs"][3])]
    assert X.loss_values(xs, b01) == [X.loss_mean(X.matvec(x), b01) for x in xs]


def test_lanczos_reorth_is_orthonormal(f8_op):
    _, X, w, g = f8_op
    V, al, _, info = X.lanczos(w, g, 20, reorth=True)
    Vh = h(V)[:info.m_eff]
    assert info.m_eff == 20
    assert np.abs(Vh @ Vh.T - np.eye(info.m_eff)).max() < 1e-12


def test_graph_replay_bitwise(f8):
    A = golden_csr(f8)
    X = dense_handle(A)
    Ax = X.matvec(t(f8["x"]))
    w, g = X.weights(Ax), X.gradient(Ax, t(f8["b01"]))
    V = torch.empty((10, X.d), dtype=X.dtype, device=DEV)
    X.set_graph(False)
    for _ in range(2):
        _, al0, be0, _ = X.lanczos(w, g, 10, V=V)
    V0 = V.clone()
    X.set_graph(True)
    for k in range(3):   # eager (new key) -> record + launch -> replay
        _, al, be, _ = X.lanczos(w, g, 10, V=V)
        np.testing.assert_array_equal(al, al0, err_msg=f"call {k}")
        np.testing.assert_array_equal(be, be0, err_msg=f"call {k}")
        assert torch.equal(V, V0), k


def test_coord_hessian_unchanged_by_the_format(f8, f8_op):
    A, X, _, _ = f8_op
    Ax = X.matvec(t(f8["x"]))
    auto = krcn.DeviceCSR(A)
    cols = np.arange(A.shape[1])
    np.testing.assert_array_equal(X.coord_hessian(cols, Ax), auto.coord_hessian(cols, Ax))


# ---------------------------------------------------------------- 7. ownership
@pytest.mark.parametrize("dtype,vs", [(torch.float64, 8), (torch.float32, 4)])
def test_images_are_owned_and_released(dtype, vs):
    """The wave plans that replace the images own tables of their own (a 32-byte descriptor
    per 512-nonzero tile), so "falls by at least 2 n d sizeof(T)" can only be asked where the
    images' padding to whole vectors outweighs them: 301 x 301 at 10 % fill pads 602 rows by
    1 (fp64) or 3 (fp32) entries, 4.8 / 7.2 KB, against ~36 tiles, 1.2 KB."""
    A, b = synth.make_dense_problem(301, 301, 0.1, seed=8)
    n, d = A.shape
    X = krcn.DeviceCSR(A, dtype=dtype, fmt=DENSE)
    b0 = X.owned_bytes()
    X.plan_info()
    b1 = X.owned_bytes()
    assert b1 - b0 >= 2 * n * d * vs
    X.reserve(10)
    b2 = X.owned_bytes()
    Ax = X.matvec(t(np.random.default_rng(3).uniform(-0.3, 0.3, d), dtype))
    X.lanczos(X.weights(Ax), X.gradient(Ax, t(O.labels01(b), dtype)), 10)
    torch.cuda.synchronize()
    assert X.owned_bytes() == b2
    X.set_format(_lib.KRCN_FORMAT_WAVE)
    X.plan_info()
    assert X.plan_format() == {"pass1": "wave", "pass2": "wave"}
    assert X.owned_bytes() <= b2 - 2 * n * d * vs


# ---------------------------------------------------------------- 8. refusals
def test_sharded_handles_refuse(f8):
    A = golden_csr(f8)
    with pytest.raises(_lib.KrcnError) as e:
        krcn.DeviceCSR(A, shard_mode=_lib.KRCN_SHARD_ROWS, fmt=DENSE)
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    X = krcn.DeviceCSR(A, shard_mode=_lib.KRCN_SHARD_ROWS)
    with pytest.raises(_lib.KrcnError) as e:
        X.set_pass_format(2, DENSE)
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED


def test_images_larger_than_the_device_refuse():
    n, d = 200_000, 2_000_000
    rows = np.arange(10) * 19_999
    cols = np.arange(10) * 199_999
    A = sp.csr_matrix((np.linspace(0.1, 1.0, 10), (rows, cols)), shape=(n, d))
    X = krcn.DeviceCSR(A, fmt=DENSE)
    b0 = X.owned_bytes()
    with pytest.raises(_lib.KrcnError) as e:
        X.plan_info()
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    msg = str(e.value)
    assert str(2 * n * d * 8) in msg
    free = re.search(r"(\d+) bytes free", msg)
    assert free and 0 < int(free.group(1)) < 2 * n * d * 8
    assert X.owned_bytes() == b0
    X.set_format(_lib.KRCN_FORMAT_AUTO)    # the handle still works with a CSR plan
    v = np.zeros(d)
    v[cols] = 1.0
    assert rel_err(h(X.matvec(t(v))), A @ v) < 1e-13


def test_unknown_format_still_raises(f8):
    X = krcn.DeviceCSR(golden_csr(f8))
    with pytest.raises(_lib.KrcnError) as e:
        X.set_format(6)
    assert e.value.status == _lib.KRCN_ERR_INVALID
    with pytest.raises(_lib.KrcnError):
        X.set_pass_format(1, 6)
