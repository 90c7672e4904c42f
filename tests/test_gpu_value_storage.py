"""fp32 value storage of the dense plans on fp64 handles (KRCN_VALUES_F32 /
KRCN_VALUES_F32_EXACT, krcn_csr_set_value_storage): a narrowed pass computes
with A32 = double(float(A)) in fp64 and nothing else.

The golden problem (tests/golden/f9_dense_values32.npz, made by
make_golden_dense_values32.py from the reference) is f8's with A32 for A.  The
handles are given f8's UNROUNDED matrix: the rounding is the library's.
Tolerances against f9 are those test_gpu_dense.py holds against f8: rel 1e-13
(max-norm) for Ax, weights, gradient, loss and HVP, 1e-11 for Lanczos alphas /
betas, 1e-6 for V, 1e-10 for the Krylov-CRN trajectory.  f9 and f8 differ by
2.4e-8 (HVP), so a pass that did not narrow misses f9 by five orders.
Every test builds the plans (plan_info) before its first compute call.
"""
import ctypes

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
F64, F32 = 0, 1


def t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def h(x):
    torch.cuda.synchronize()
    return x.cpu().numpy()


def a32(A):
    """A with every value rounded to fp32 and widened back."""
    return sp.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices.copy(), A.indptr.copy()),
                         shape=A.shape)


def dense_handle(A, **kw):
    kw.setdefault("fmt", DENSE)
    X = krcn.DeviceCSR(A, **kw)
    X.plan_info()   # images built here, never inside a compute call
    return X


def geometry(rows, cols, dtype, lanes=0, slicing=0):
    out = (ctypes.c_int64 * 8)()
    _lib.call("krcn_dense_geometry", rows, cols, dtype, lanes, slicing, out)
    return dict(zip(("ld", "L", "S", "width", "groups", "grid", "bytes", "nvec"), (int(v) for v in out)))


def plan_of(g):
    return (g["S"], g["L"], g["groups"], g["grid"])


@pytest.fixture(scope="module")
def f8():
    return load_golden("f8_dense.npz")


@pytest.fixture(scope="module")
def f9():
    return load_golden("f9_dense_values32.npz")


@pytest.fixture(scope="module")
def f9_op(f8, f9):
    """(A32, narrowed handle built from f8's unrounded matrix, w, g) at the golden x; shared read-only."""
    X = dense_handle(golden_csr(f8), values="f32")
    Ax = X.matvec(t(f9["x"]))
    return golden_csr(f9), X, X.weights(Ax), X.gradient(Ax, t(f9["b01"]))


# ------------------------------------------------------------ 1. against f9
def test_objective_pieces_vs_golden(f8, f9, f9_op):
    A32, X, _, _ = f9_op
    assert X.plan_format() == {"pass1": "dense", "pass2": "dense"}
    assert X.plan_value_bytes() == {"pass1": 4, "pass2": 4}
    n, d = A32.shape
    assert X.plan_info() == {"pass1": plan_of(geometry(n, d, F32)), "pass2": plan_of(geometry(d, n, F32))}
    x, b01 = t(f9["x"]), t(f9["b01"])
    Ax = X.matvec(x)
    assert rel_err(h(Ax), f9["Ax_l2_0"]) < 1e-13
    w = X.weights(Ax)
    assert rel_err(h(w), O.hessian_weights(A32, f9["x"])) < 1e-13
    assert rel_err(h(X.gradient(Ax, b01)), f9["grad_l2_0"]) < 1e-13
    assert rel_err(h(X.gradient(Ax, b01, x, l2=0.01)), f9["grad_l2_1"]) < 1e-13
    assert abs(X.loss_mean(Ax, b01) - f9["value_l2_0"]) < 1e-13 * abs(f9["value_l2_0"])
    for k in range(3):
        v = t(f9[f"v{k}"])
        y = h(X.hvp(w, v))
        assert rel_err(y, f9[f"hvp{k}_l2_0"]) < 1e-13
        assert rel_err(h(X.hvp(w, v, l2=0.01)), f9[f"hvp{k}_l2_1"]) < 1e-13
        assert rel_err(y, f8[f"hvp{k}_l2_0"]) > 1e-10   # the narrowing happened


@pytest.mark.parametrize("m", [10, 20])
def test_lanczos_vs_golden(f9, f9_op, m):
    _, X, w, g = f9_op
    V, al, be, info = X.lanczos(w, g, m)
    assert info.m_eff == m and not info.breakdown
    assert rel_err(al, f9[f"alphas_m{m}"]) < 1e-11
    assert rel_err(be, f9[f"betas_m{m}"]) < 1e-11
    assert rel_err(h(V).T, f9[f"V_m{m}"]) < 1e-6


def test_krylov_crn_trajectory_vs_golden(f8, f9):
    A = golden_csr(f8)
    loss = LogisticRegression(A, f8["b"], l1=0, l2=0, store_mat_vec_prod=True, format="dense", values="f32")
    assert loss.device_matrix.plan_format() == {"pass1": "dense", "pass2": "dense"}
    assert loss.device_matrix.plan_value_bytes() == {"pass1": 4, "pass2": 4}
    opt = Cubic_Krylov_LS(loss=loss, reg_coef=1e-3, label="krylov", subspace_dim=10, tolerance=1e-9, tqdm=False)
    tr = opt.run(x0=np.full(A.shape[1], 0.5), it_max=8)
    opt.compute_loss_of_iterates()
    xs = np.asarray(tr.xs)
    assert xs.shape == f9["crn_xs"].shape
    assert rel_err(xs, f9["crn_xs"]) < 1e-10
    assert tr.solver_its == list(f9["crn_solver_its"])
    np.testing.assert_allclose(tr.loss_vals, f9["crn_loss_vals"], rtol=1e-10)
    assert opt.reg_coef == f9["crn_final_reg_coef"]


def test_loss_values_argument(f8):
    A = golden_csr(f8)
    for bad in ("f32", "f32-exact"):
        with pytest.raises(ValueError):
            LogisticRegression(A, f8["b"], l1=0, l2=0, values=bad)
        with pytest.raises(ValueError):
            LogisticRegression(A, f8["b"], l1=0, l2=0, format=_lib.KRCN_FORMAT_WAVE, values=bad)
    with pytest.raises(ValueError):
        LogisticRegression(A, f8["b"], l1=0, l2=0, format="dense", values="f16")
    full = LogisticRegression(A, f8["b"], l1=0, l2=0, format="dense", values="full")
    assert full.device_matrix.plan_value_bytes() == {"pass1": 8, "pass2": 8}
    exact = LogisticRegression(A, f8["b"], l1=0, l2=0, format="dense", values="f32-exact")
    assert exact.device_matrix.plan_value_bytes() == {"pass1": 8, "pass2": 8}   # no value of f8 is fp32-exact
    assert LogisticRegression(A, f8["b"], l1=0, l2=0).device_matrix.plan_value_bytes() == {"pass1": 8, "pass2": 8}


# -------------------------------- 2. the sequential policy is bitwise scipy on A32
def signed_zero_problem():
    A, _ = synth.make_dense_problem(67, 129, 0.9, seed=3)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(129)
    u = rng.standard_normal(67)
    v[[0, 7, 64, 128]] = [0.0, -0.0, -0.0, 0.0]
    u[[0, 33, 66]] = [-0.0, 0.0, -0.0]
    return A, u, v, rng.uniform(0.01, 0.25, 67)


def test_sequential_policy_is_bitwise_scipy_on_a32(f8):
    A8 = golden_csr(f8)
    rng = np.random.default_rng(9)
    cases = [(A8, rng.standard_normal(130), f8["v0"], O.hessian_weights(a32(A8), f8["x"])), signed_zero_problem()]
    for A, u, v, w in cases:
        X = dense_handle(A, lanes=(1, 1), values="f32")
        assert X.plan_value_bytes() == {"pass1": 4, "pass2": 4}
        assert X.plan_info() == {"pass1": (1, 1, -(-A.shape[0] // 256), -(-A.shape[0] // 256)),
                                 "pass2": (1, 1, -(-A.shape[1] // 256), -(-A.shape[1] // 256))}
        B = a32(A)
        assert not np.array_equal(B.data, A.data)
        np.testing.assert_array_equal(h(X.matvec(t(v))), B @ v)
        np.testing.assert_array_equal(h(X.rmatvec(t(u))), (B.T @ u) / B.shape[0])
        np.testing.assert_array_equal(h(X.hvp(t(w), t(v))), O.hvp_from_weights(B, w, v))


# ----------------------------------------------------------- 3. edge shapes
def check_passes(A, X, ref=None, seed=1):
    """Both passes and the HVP of X (holding A) against the oracle on `ref` (default A32) at 1e-13."""
    n, d = A.shape
    B = a32(A) if ref is None else ref
    rng = np.random.default_rng(seed)
    u, v, w = rng.standard_normal(n), rng.standard_normal(d), rng.uniform(0.01, 0.25, n)
    assert rel_err(h(X.matvec(t(v))), B @ v) < 1e-13
    assert rel_err(h(X.rmatvec(t(u))), (B.T @ u) / n) < 1e-13
    assert rel_err(h(X.hvp(t(w), t(v))), O.hvp_from_weights(B, w, v)) < 1e-13
    assert rel_err(h(X.hvp(t(w), t(v), l2=0.01)), O.hvp_from_weights(B, w, v, 0.01)) < 1e-13


def narrowed(A, X):
    """The handle's passes tell A32 from A (skipped where rounding cannot show: never here)."""
    v = np.random.default_rng(1).standard_normal(A.shape[1])
    return rel_err(h(X.matvec(t(v))), A @ v) > 1e-10


# column counts around whole vectors (4 entries) and tail vectors of 1..3; (3, 130): fewer rows than a row group
EDGE = [(9, 1), (9, 3), (9, 4), (9, 5), (67, 129), (67, 130), (67, 131), (3, 130), (130, 3), (300, 257)]


@pytest.mark.parametrize("n,d", EDGE)
def test_edge_shapes(n, d):
    A, _ = synth.make_dense_problem(n, d, 0.9, seed=100 + n + d)
    for lanes in (0, 2, 8, 64):
        X = dense_handle(A, lanes=(lanes, lanes), values="f32")
        assert X.plan_format() == {"pass1": "dense", "pass2": "dense"}
        assert X.plan_value_bytes() == {"pass1": 4, "pass2": 4}
        assert X.plan_info() == {"pass1": plan_of(geometry(n, d, F32, lanes)),
                                 "pass2": plan_of(geometry(d, n, F32, lanes))}
        if lanes:
            info = X.plan_info()
            assert info["pass1"][1] == lanes and info["pass2"][1] == lanes
        check_passes(A, X)
        assert narrowed(A, X)


def test_empty_matrix():
    A = sp.csr_matrix((5, 6), dtype=np.float64)
    X = dense_handle(A, values="f32")
    assert X.plan_value_bytes() == {"pass1": 4, "pass2": 4}
    check_passes(A, X)


def test_stored_zeros_and_unsorted_columns():
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
            X = dense_handle(M, lanes=(lanes, lanes), values="f32")
            check_passes(M, X)
            assert narrowed(M, X)


def test_forced_slices_pass1():
    """12 rows of 2,100 (525 four-entry vectors) in 8 slices.  The Lanczos point is that of
    test_gpu_dense.py::test_forced_slices_pass1 (x within +-0.2, weights over 0.004..0.16, where
    reordered sums move the oracle's alphas and betas by <= 6e-15), m = 10."""
    A, b = synth.make_dense_problem(12, 2100, 0.95, seed=6)
    X = dense_handle(A, slicing=8, values="f32")
    info = X.plan_info()
    assert info["pass1"][0] == 8 and info["pass1"][3] % 8 == 0
    assert info == {"pass1": plan_of(geometry(12, 2100, F32, 0, 8)), "pass2": plan_of(geometry(2100, 12, F32, 0, 8))}
    check_passes(A, X)
    assert narrowed(A, X)
    B = a32(A)
    x = np.random.default_rng(2).uniform(-0.2, 0.2, 2100)
    w = O.hessian_weights(B, x)
    g = O.gradient(B, O.labels01(b), x)
    _, al, be, info = X.lanczos(t(w), t(g), 10)
    _, alr, ber, _ = O.lanczos(lambda q: O.hvp_from_weights(B, w, q), g, m=10)
    assert info.m_eff == 10
    assert rel_err(al, alr) < 1e-11
    assert rel_err(be, ber) < 1e-11


def test_forced_slices_pass2():
    A, _ = synth.make_dense_problem(2100, 12, 0.95, seed=7)
    X = dense_handle(A, slicing=8, values="f32")
    info = X.plan_info()
    assert info["pass2"][0] == 8 and info["pass1"][0] < 8    # pass 1: 12 columns are 3 vectors
    check_passes(A, X)
    assert narrowed(A, X)


def test_auto_slices_few_long_rows():
    A, _ = synth.make_dense_problem(12, 2100, 0.95, seed=6)
    X = dense_handle(A, values="f32")
    assert X.plan_info()["pass1"][0] > 1 and X.plan_info()["pass2"][0] == 1
    assert X.plan_info()["pass1"] == plan_of(geometry(12, 2100, F32))
    check_passes(A, X)
    assert narrowed(A, X)


def test_lanczos_unaligned_basis_rows():
    """d = 129: the basis rows at odd j start 8 bytes off a 16-byte boundary, so pass 1 gathers
    them with guarded scalar loads.  The weights come from x within +-0.2 (the range
    test_gpu_dense.py::test_forced_slices_pass1 explains), m = 5."""
    A, b = synth.make_dense_problem(67, 129, 0.9, seed=3)
    B = a32(A)
    x = np.random.default_rng(2).uniform(-0.2, 0.2, 129)
    w = O.hessian_weights(B, x)
    g = O.gradient(B, O.labels01(b), x)
    _, alr, ber, _ = O.lanczos(lambda q: O.hvp_from_weights(B, w, q), g, m=5)
    for lanes in (0, 8):
        X = dense_handle(A, lanes=(lanes, lanes), values="f32")
        V, al, be, info = X.lanczos(t(w), t(g), 5)
        assert info.m_eff == 5
        assert rel_err(al, alr) < 1e-11
        assert rel_err(be, ber) < 1e-11


# ----------------------------------------------------------------- 4. f32-exact
def outputs(X, u, v, w):
    return [h(X.matvec(t(v))), h(X.rmatvec(t(u))), h(X.hvp(t(w), t(v))), h(X.hvp(t(w), t(v), l2=0.01))]


def test_f32_exact(f9):
    B = golden_csr(f9)                          # every value fp32-exact
    data = B.data.copy()
    data[1234] = 0.1                            # ... but this one
    C = sp.csr_matrix((data, B.indices, B.indptr), shape=B.shape)
    assert np.float64(np.float32(0.1)) != 0.1
    rng = np.random.default_rng(4)
    u, v, w = rng.standard_normal(130), rng.standard_normal(75), rng.uniform(0.01, 0.25, 130)
    for lanes in (0, 1):
        got = {}
        for M, name in ((B, "exact"), (C, "inexact")):
            for values in ("full", "f32", "f32-exact"):
                X = dense_handle(M, lanes=(lanes, lanes), values=values)
                got[name, values] = (X.plan_value_bytes(), X.plan_info(), outputs(X, u, v, w))
        for name, like, nbytes in (("exact", "f32", 4), ("inexact", "full", 8)):
            vb, info, ys = got[name, "f32-exact"]
            assert vb == {"pass1": nbytes, "pass2": nbytes}, (name, lanes)
            assert (vb, info) == got[name, like][:2]
            for y, y0 in zip(ys, got[name, like][2]):
                np.testing.assert_array_equal(y, y0)
        if lanes == 1:   # one left-to-right sum per row over the same numbers, whatever their stored width
            for y, y0 in zip(got["exact", "f32-exact"][2], got["exact", "full"][2]):
                np.testing.assert_array_equal(y, y0)


def test_f32_exact_nan_keeps_full(f9):
    B = golden_csr(f9)
    data = B.data.copy()
    data[77] = np.nan
    X = dense_handle(sp.csr_matrix((data, B.indices, B.indptr), shape=B.shape), values="f32-exact")
    assert X.plan_value_bytes() == {"pass1": 8, "pass2": 8}


# --------------------------------------------------------------------- 5. bytes
def test_images_are_owned_and_released():
    """As test_gpu_dense.py::test_images_are_owned_and_released: 301 x 301 at 10 % fill, where the
    images' padding outweighs the tables of the wave plans that replace them."""
    A, b = synth.make_dense_problem(301, 301, 0.1, seed=8)
    n, d = A.shape
    want32 = geometry(n, d, F32)["bytes"] + geometry(d, n, F32)["bytes"]
    want64 = geometry(n, d, F64)["bytes"] + geometry(d, n, F64)["bytes"]
    assert want32 == 2 * 301 * 304 * 4 and want64 == 2 * 301 * 302 * 8
    # a handle's first plan build also allocates its partials buffers, whatever the stored width:
    # a full-width twin measures them, so that the images' bytes are held to the geometry's exactly
    twin = krcn.DeviceCSR(A, fmt=DENSE)
    t0 = twin.owned_bytes()
    twin.plan_info()
    workspace = twin.owned_bytes() - t0 - want64
    assert 0 <= workspace < 1 << 20
    twin.close()
    X = krcn.DeviceCSR(A, fmt=DENSE, values="f32")
    b0 = X.owned_bytes()
    X.plan_info()
    b1 = X.owned_bytes()
    assert b1 - b0 - workspace == want32
    X.reserve(10)
    b2 = X.owned_bytes()
    Ax = X.matvec(t(np.random.default_rng(3).uniform(-0.3, 0.3, d)))
    X.lanczos(X.weights(Ax), X.gradient(Ax, t(O.labels01(b))), 10)
    torch.cuda.synchronize()
    assert X.owned_bytes() == b2
    X.set_value_storage("full")
    X.plan_info()
    assert X.plan_value_bytes() == {"pass1": 8, "pass2": 8}
    assert X.owned_bytes() - b2 == want64 - want32
    X.set_value_storage("f32")
    X.plan_info()
    assert X.owned_bytes() == b2
    X.set_format(_lib.KRCN_FORMAT_WAVE)
    X.plan_info()
    assert X.plan_format() == {"pass1": "wave", "pass2": "wave"}
    assert X.plan_value_bytes() == {"pass1": 8, "pass2": 8}
    assert X.owned_bytes() <= b2 - 2 * n * d * 4
    X.set_format(DENSE)
    X.plan_info()
    assert X.owned_bytes() == b2               # narrowed again: the same bytes as before
    X.close()                                  # (the owner tables free what owned_bytes counted)
    assert X.handle.value is None
    X.close()


# ---------------------------------------------------------------- 6. boundaries
def test_fp32_handle_policy_is_a_no_op(f8):
    A = golden_csr(f8)
    rng = np.random.default_rng(4)
    u, v, w = (t(a, torch.float32) for a in (rng.standard_normal(130), rng.standard_normal(75),
                                             rng.uniform(0.01, 0.25, 130)))
    got = []
    for values in ("full", "f32", "f32-exact"):
        X = dense_handle(A, dtype=torch.float32, values=values)
        assert X.plan_value_bytes() == {"pass1": 4, "pass2": 4}
        got.append((X.plan_info(), X.owned_bytes(), h(X.matvec(v)), h(X.rmatvec(u)), h(X.hvp(w, v))))
    for g in got[1:]:
        assert g[:2] == got[0][:2]
        for y, y0 in zip(g[2:], got[0][2:]):
            np.testing.assert_array_equal(y, y0)
    wave = krcn.DeviceCSR(A, dtype=torch.float32, values="f32")
    assert wave.plan_value_bytes() == {"pass1": 4, "pass2": 4}


def test_mixed_passes_narrow_the_dense_one_only(f8):
    A = golden_csr(f8)
    B = a32(A)
    rng = np.random.default_rng(1)
    u, v = rng.standard_normal(130), rng.standard_normal(75)
    X = krcn.DeviceCSR(A, pass_formats=(5, 1), values="f32")
    X.plan_info()
    assert X.plan_format() == {"pass1": "dense", "pass2": "wave"}
    assert X.plan_value_bytes() == {"pass1": 4, "pass2": 8}
    assert rel_err(h(X.matvec(t(v))), B @ v) < 1e-13
    assert rel_err(h(X.rmatvec(t(u))), (A.T @ u) / 130) < 1e-13
    X = krcn.DeviceCSR(A, pass_formats=(1, 5), values="f32")
    X.plan_info()
    assert X.plan_value_bytes() == {"pass1": 8, "pass2": 4}
    assert rel_err(h(X.matvec(t(v))), A @ v) < 1e-13
    assert rel_err(h(X.rmatvec(t(u))), (B.T @ u) / 130) < 1e-13


def test_invalid_value_raises_and_leaves_the_plans_usable(f9, f9_op):
    _, X, w, _ = f9_op
    info = X.plan_info()
    for bad in (3, -1):
        with pytest.raises(_lib.KrcnError) as e:
            X.set_value_storage(bad)
        assert e.value.status == _lib.KRCN_ERR_INVALID
    with pytest.raises(ValueError):
        X.set_value_storage("f16")
    assert _lib.load().krcn_csr_plan_value_bytes(X.handle, None) == _lib.KRCN_ERR_INVALID
    assert X.plan_value_bytes() == {"pass1": 4, "pass2": 4} and X.plan_info() == info
    assert rel_err(h(X.hvp(w, t(f9["v0"]))), f9["hvp0_l2_0"]) < 1e-13


def test_sharded_handles_refuse(f8):
    A = golden_csr(f8)
    X = krcn.DeviceCSR(A, shard_mode=_lib.KRCN_SHARD_ROWS)
    for values in ("f32", "f32-exact"):
        with pytest.raises(_lib.KrcnError) as e:
            X.set_value_storage(values)
        assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    X.set_value_storage("full")
    assert X.plan_value_bytes() == {"pass1": 8, "pass2": 8}
    with pytest.raises(_lib.KrcnError) as e:
        krcn.DeviceCSR(A, shard_mode=_lib.KRCN_SHARD_ROWS, values="f32")
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED


def test_coord_hessian_reads_full_width_values(f8, f9_op):
    _, X, _, _ = f9_op
    A = golden_csr(f8)
    full = dense_handle(A)
    Ax = full.matvec(t(f8["x"]))
    cols = np.arange(A.shape[1])
    np.testing.assert_array_equal(X.coord_hessian(cols, Ax), full.coord_hessian(cols, Ax))
    _, _, vals = X.transpose_arrays()
    np.testing.assert_array_equal(np.sort(h(vals)), np.sort(A.data))


def test_graph_replay_bitwise(f8, f9):
    X = dense_handle(golden_csr(f8), values="f32")
    Ax = X.matvec(t(f9["x"]))
    w, g = X.weights(Ax), X.gradient(Ax, t(f9["b01"]))
    V = torch.empty((10, X.d), dtype=X.dtype, device=DEV)
    X.set_graph(False)
    for _ in range(2):
        _, al0, be0, _ = X.lanczos(w, g, 10, V=V)
    assert rel_err(al0, f9["alphas_m10"]) < 1e-11
    V0 = V.clone()
    X.set_graph(True)
    for k in range(3):   # eager (new key) -> record + launch -> replay
        _, al, be, _ = X.lanczos(w, g, 10, V=V)
        np.testing.assert_array_equal(al, al0, err_msg=f"call {k}")
        np.testing.assert_array_equal(be, be0, err_msg=f"call {k}")
        assert torch.equal(V, V0), k


def test_loss_values_bitwise(f9, f9_op):
    _, X, _, _ = f9_op
    b01 = t(f9["b01"])
    xs = [t(f9["x"]), t(f9["v0"] * 0.1), t(f9["crn_xs"][3])]
    assert X.loss_values(xs, b01) == [X.loss_mean(X.matvec(x), b01) for x in xs]


def test_cg_solve_matches_dense_solve(f9, f9_op):
    A32, X, _, _ = f9_op
    w = O.hessian_weights(A32, f9["x"])
    rhs = np.random.default_rng(2).standard_normal(A32.shape[1])
    shift = 0.05
    sol, info = X.cg_solve(t(w), t(rhs), shift=shift, rtol=1e-10)
    H = (A32.T.multiply(w) @ A32 / A32.shape[0]).toarray() + shift * np.eye(A32.shape[1])
    assert info.converged == 1 and info.info == 0 and 0 < info.iterations < 10 * A32.shape[1]
    assert info.residual_norm < 1e-10 * np.linalg.norm(rhs)
    assert rel_err(h(sol), np.linalg.solve(H, rhs)) < 1e-8
