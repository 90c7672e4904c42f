"""Block products (krcn_matvec_block / krcn_rmatvec_block / krcn_hvp_block): k
vectors per pass over the matrix, against scipy / numpy on the host.

Bitwise (fp64): a row of at most KRCN_BLOCK_LONG_ROW stored elements is summed
left to right, product and sum rounded separately: scipy's csr_matvecs order on
X and csc_matvecs order on X^T.  The matrices of the bitwise tests hold no
longer row (checked on the CPU below), so nothing is excluded from them.
Longer rows are summed by segments in a fixed order: 1e-13 (conftest.rel_err,
the suite's HVP bound), byte-identical from run to run and whatever the
neighbouring rows are.  fp32 handles: 1e-5 (the suite's fp32 HVP bound).

The grid of a pass is ceil(rows / (256 / K)) workgroups with no cap, K the
next power of two >= k, so there is no grid-cap case; the sizes below walk the
row counts around 64 / K rows a wave and 256 / K rows a workgroup for every K.
Which rows count as long is decided on the host (csrc/krcn_block_rows.hpp,
checked under the host sanitizers by tests/test_block_rows.py).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
import krcn_oracle as O
from conftest import golden_csr, rel_err
from krcn import _lib
from optimizer.loss import LogisticRegression

gpu = pytest.mark.gpu
DEV = "cuda"
LONG = _lib.KRCN_BLOCK_LONG_ROW
KS = (1, 2, 3, 5, 8, 13, 16)
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257)


def t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def h(x):
    return x.detach().cpu().numpy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def status_of(exc):
    return exc.value.status


# ------------------------------------------------------------------ matrices
def random_matrix():
    rng = np.random.default_rng(20)
    A = sp.random(301, 419, density=0.03, random_state=rng, format="csr",
                  data_rvs=lambda s: rng.uniform(-1.0, 1.0, s))
    A.sort_indices()
    return A


def edge_matrix(n, d, seed):
    """One to six nonzeros a row (at most d), empty first and last rows."""
    rng = np.random.default_rng(seed)
    indptr, indices = [0], []
    for r in range(n):
        cnt = 0 if (n >= 3 and r in (0, n - 1)) else min(int(rng.integers(1, 7)), d)
        indices.extend(sorted(rng.choice(d, cnt, replace=False).tolist()))
        indptr.append(len(indices))
    data = rng.uniform(-1.0, 1.0, len(indices))
    return sp.csr_matrix((data, np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(n, d))


LONG_LENS = (LONG, LONG + 1, 3 * LONG + 7, 20000)
LONG_N, LONG_D = 48, 20011


def long_matrix(positions, seed):
    """LONG_N x LONG_D: rows of LONG_LENS elements at `positions` (their content
    does not depend on positions or seed), short rows from `seed` elsewhere."""
    fixed = np.random.default_rng(99)
    longs = []
    for ln in LONG_LENS:
        cols = np.sort(fixed.choice(LONG_D, ln, replace=False))
        longs.append((cols, fixed.uniform(-1.0, 1.0, ln)))
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for r in range(LONG_N):
        if r in positions:
            cols, vals = longs[positions.index(r)]
        else:
            cnt = int(rng.integers(0, 7))
            cols = np.sort(rng.choice(LONG_D, cnt, replace=False))
            vals = rng.uniform(-1.0, 1.0, cnt)
        indices.extend(cols.tolist())
        data.extend(vals.tolist())
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)),
                         shape=(LONG_N, LONG_D))


POS_A, POS_B = (3, 7, 12, 20), (0, 30, 31, 47)


def row_lengths(A):
    return np.diff(A.indptr), np.diff(A.T.tocsr().indptr)


def block_inputs(A, k, seed=5):
    n, d = A.shape
    rng = np.random.default_rng(seed + 100 * k)
    V = rng.standard_normal((d, k))
    U = rng.standard_normal((n, k))
    w1 = rng.uniform(0.05, 0.25, n)
    wk = rng.uniform(0.05, 0.25, (n, k))
    return V, U, w1, wk


def host_hvp(A, w, V, l2):
    W = w[:, None] if w.ndim == 1 else w
    return A.T @ (W * (A @ V)) / A.shape[0] + np.asarray(l2, dtype=np.float64) * V


def mixed_l2(k):
    return np.array([0.0 if j % 2 else 0.01 * (j + 1) for j in range(k)])


@pytest.fixture(scope="module")
def mats(f1):
    return {"f1": golden_csr(f1), "random": random_matrix()}


@pytest.fixture(scope="module")
def handles(mats):
    return {name: krcn.DeviceCSR(A) for name, A in mats.items()}


# ------------------------------------------------------------- CPU: the cases
def test_bitwise_matrices_hold_no_long_row(f1):
    for A in (golden_csr(f1), random_matrix()):
        rx, rxt = row_lengths(A)
        assert rx.max() <= LONG and rxt.max() <= LONG
    for i, n in enumerate(SIZES):
        rx, rxt = row_lengths(edge_matrix(n, SIZES[-1 - i], seed=i))
        assert rx.max() <= 6 and rxt.max() <= LONG
        if n >= 3:
            assert rx[0] == 0 and rx[-1] == 0


def test_long_row_matrices():
    A, B = long_matrix(list(POS_A), 1), long_matrix(list(POS_B), 2)
    for M, pos in ((A, POS_A), (B, POS_B)):
        rx, rxt = row_lengths(M)
        assert tuple(rx[list(pos)]) == LONG_LENS
        assert np.delete(rx, list(pos)).max() <= 6 and rxt.max() <= LONG_N
    for pa, pb in zip(POS_A, POS_B):   # the same row among different neighbours
        assert np.array_equal(A[pa].indices, B[pb].indices) and np.array_equal(A[pa].data, B[pb].data)
    assert not np.array_equal(A[0].indices, B[1].indices)


# ------------------------------------------------------------- bitwise, fp64
@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["f1", "random"])
def test_bitwise_vs_scipy(mats, handles, name, k):
    A, X = mats[name], handles[name]
    n = A.shape[0]
    rx, rxt = row_lengths(A)
    assert rx.max() <= LONG and rxt.max() <= LONG
    V, U, w1, wk = block_inputs(A, k)
    assert same_bytes(h(X.matvec_block(t(V))), A @ V)
    assert same_bytes(h(X.rmatvec_block(t(U))), (A.T.tocsr() @ U) / n)
    for w in (w1, wk):
        for l2 in (0.0, 0.01, mixed_l2(k)):
            got = h(X.hvp_block(t(w), t(V), l2=l2))
            assert same_bytes(got, host_hvp(A, w, V, l2)), f"k {k} w {w.shape} l2 {l2}"


@gpu
@pytest.mark.parametrize("k", KS)
def test_columns_equal_the_sequential_single_hvp(mats, k):
    A = mats["f1"]
    X, Xseq = krcn.DeviceCSR(A), krcn.DeviceCSR(A, lanes=(_lib.KRCN_LANES_SEQUENTIAL, _lib.KRCN_LANES_SEQUENTIAL))
    V, _, w1, _ = block_inputs(A, k)
    for l2 in (0.0, 0.01):
        Y = h(X.hvp_block(t(w1), t(V), l2=l2))
        for j in range(k):
            assert same_bytes(Y[:, j], h(Xseq.hvp(t(w1), t(V[:, j]), l2=l2)))


# ------------------------------------------- lane-group and partition edges
@gpu
@pytest.mark.parametrize("i", range(len(SIZES)))
def test_row_count_edges(i):
    n, d = SIZES[i], SIZES[-1 - i]
    A = edge_matrix(n, d, seed=i)
    X = krcn.DeviceCSR(A)
    At = A.T.tocsr()
    for k in KS:
        V, U, _, wk = block_inputs(A, k)
        assert same_bytes(h(X.matvec_block(t(V))), A @ V), f"n {n} d {d} k {k}"
        assert same_bytes(h(X.rmatvec_block(t(U))), (At @ U) / n), f"n {n} d {d} k {k}"
        l2 = mixed_l2(k)
        assert same_bytes(h(X.hvp_block(t(wk), t(V), l2=l2)), host_hvp(A, wk, V, l2)), f"n {n} d {d} k {k}"


# ------------------------------------------------------------------ long rows
@gpu
@pytest.mark.parametrize("side", ["x", "xt"])
def test_long_rows(side):
    A, B = long_matrix(list(POS_A), 1), long_matrix(list(POS_B), 2)
    if side == "xt":
        A, B = A.T.tocsr(), B.T.tocsr()
    X, X2 = krcn.DeviceCSR(A), krcn.DeviceCSR(B)
    n = A.shape[0]
    pa, pb = list(POS_A), list(POS_B)
    # the long-row list: 4 bytes for each of the three rows above the threshold, on the side that has them
    fresh = X.owned_bytes()
    X.matvec_block(t(np.ones((A.shape[1], 2))))
    assert X.owned_bytes() - fresh == (12 if side == "x" else 0)
    X.rmatvec_block(t(np.ones((n, 2))))
    assert X.owned_bytes() - fresh == 12
    for k in (1, 2, 3, 8, 16):
        V, U, w1, _ = block_inputs(A, k)
        Vd, Ud, wd = t(V), t(U), t(w1)
        Tn, Y, Hv = h(X.matvec_block(Vd)), h(X.rmatvec_block(Ud)), h(X.hvp_block(wd, Vd, l2=0.01))
        eT, eY = A @ V, (A.T.tocsr() @ U) / n
        # the product whose rows are long: at or below the threshold bitwise, above it 1e-13
        got, exp = (Tn, eT) if side == "x" else (Y, eY)
        short = np.ones(got.shape[0], dtype=bool)
        short[pa[1:]] = False
        assert same_bytes(got[short], exp[short]), f"{side} k {k}"
        e_long = rel_err(got, exp)
        e_hvp = rel_err(Hv, host_hvp(A, w1, V, 0.01))
        print(f"{side} k {k}: long-row product rel err {e_long:.3e}, hvp rel err {e_hvp:.3e}")
        assert e_long < 1e-13
        assert e_hvp < 1e-13
        # the other product has short rows only
        assert same_bytes(*((Y, eY) if side == "x" else (Tn, eT)))
        # run to run
        assert same_bytes(Tn, h(X.matvec_block(Vd)))
        assert same_bytes(Y, h(X.rmatvec_block(Ud)))
        assert same_bytes(Hv, h(X.hvp_block(wd, Vd, l2=0.01)))
        # the same rows among other neighbours, at other places of their workgroup
        got2 = h(X2.matvec_block(Vd)) if side == "x" else h(X2.rmatvec_block(Ud))
        assert same_bytes(got2[pb], got[pa]), f"{side} k {k}: a long row's sum depends on its neighbours"


# ------------------------------------------------------- column independence
@gpu
@pytest.mark.parametrize("k", [3, 5, 8, 16])
def test_columns_do_not_mix(mats, handles, k):
    A, X = mats["f1"], handles["f1"]
    V, U, w1, _ = block_inputs(A, k)
    Vb, Ub = V.copy(), U.copy()
    Vb[:, 0], Vb[:, k - 1] = np.nan, np.inf
    Ub[:, 0], Ub[:, k - 1] = np.nan, np.inf
    mid = slice(1, k - 1)
    assert same_bytes(h(X.matvec_block(t(Vb)))[:, mid], h(X.matvec_block(t(V)))[:, mid])
    assert same_bytes(h(X.rmatvec_block(t(Ub)))[:, mid], h(X.rmatvec_block(t(U)))[:, mid])
    assert same_bytes(h(X.hvp_block(t(w1), t(Vb), l2=0.01))[:, mid], h(X.hvp_block(t(w1), t(V), l2=0.01))[:, mid])


@gpu
@pytest.mark.parametrize("k", [3, 5])
def test_idle_members_store_nothing(mats, handles, k):
    """k = 3, 5 run lane groups of 4, 8: outputs in the middle of NaN-filled
    buffers, whose canaries on both sides survive."""
    A, X = mats["f1"], handles["f1"]
    n, d = A.shape
    V, U, w1, _ = block_inputs(A, k)
    pad = 64

    def framed(rows):
        big = torch.full((pad + rows * k + pad,), float("nan"), dtype=torch.float64, device=DEV)
        return big, big[pad:pad + rows * k].view(rows, k)

    def canaries_alive(big):
        b = h(big)
        return np.isnan(b[:pad]).all() and np.isnan(b[-pad:]).all()

    big, out = framed(n)
    X.matvec_block(t(V), out=out)
    assert canaries_alive(big) and same_bytes(h(out), A @ V)
    big, out = framed(d)
    X.rmatvec_block(t(U), out=out)
    assert canaries_alive(big) and same_bytes(h(out), (A.T.tocsr() @ U) / n)
    big, out = framed(d)
    X.hvp_block(t(w1), t(V), l2=0.01, out=out)
    assert canaries_alive(big) and same_bytes(h(out), host_hvp(A, w1, V, 0.01))


@gpu
def test_l2_zero_column_never_reads_v(mats, handles):
    """A NaN of V at an empty column of X reaches no row sum; with l2_j == 0 the
    epilogue does not read it either, as krcn_hvp's: column j stays finite."""
    A, X = mats["f1"], handles["f1"]
    empty = np.flatnonzero(np.diff(A.T.tocsr().indptr) == 0)
    assert len(empty), "f1 has empty columns"
    k = 5
    V, _, w1, _ = block_inputs(A, k)
    V[empty[0], :] = np.nan
    l2 = np.array([0.01, 0.0, 0.01, 0.0, 0.01])
    Y = h(X.hvp_block(t(w1), t(V), l2=l2))
    for j in range(k):
        single = h(X.hvp(t(w1), t(V[:, j]), l2=float(l2[j])))
        assert np.isfinite(Y[:, j]).all() == (l2[j] == 0.0)
        assert np.array_equal(np.isfinite(Y[:, j]), np.isfinite(single))
    assert np.isnan(Y[empty[0], 0]) and Y[empty[0], 1] == 0.0


# ----------------------------------------------------------------- fp32 handle
@gpu
@pytest.mark.parametrize("k", [3, 8, 16])
def test_fp32_handle(mats, k):
    A = mats["f1"]
    n = A.shape[0]
    X = krcn.DeviceCSR(A, dtype=torch.float32)
    f32 = torch.float32
    V, U, w1, wk = (a.astype(np.float32).astype(np.float64) for a in block_inputs(A, k))
    errs = [rel_err(h(X.matvec_block(t(V, f32))), A @ V),
            rel_err(h(X.rmatvec_block(t(U, f32))), (A.T.tocsr() @ U) / n),
            rel_err(h(X.hvp_block(t(w1, f32), t(V, f32), l2=0.01)), host_hvp(A, w1, V, 0.01)),
            rel_err(h(X.hvp_block(t(wk, f32), t(V, f32), l2=mixed_l2(k))), host_hvp(A, wk, V, mixed_l2(k)))]
    print(f"fp32 k {k}: rel errs {['%.2e' % e for e in errs]}")
    assert X.matvec_block(t(V, f32)).dtype == f32
    assert max(errs) < 1e-5


# -------------------------------------------------------------------- refusals
@gpu
def test_refusals(mats, handles):
    A, X = mats["f1"], handles["f1"]
    n, d = A.shape
    w = t(np.ones(n))
    for k in (0, _lib.KRCN_BLOCK_MAX + 1):
        V, U = t(np.zeros((d, k))), t(np.zeros((n, k)))
        for fn in (lambda: X.matvec_block(V), lambda: X.rmatvec_block(U), lambda: X.hvp_block(w, V)):
            with pytest.raises(_lib.KrcnError) as e:
                fn()
            assert status_of(e) == _lib.KRCN_ERR_INVALID
    with pytest.raises(_lib.KrcnError) as e:
        X.hvp_block(t(np.ones((n, 2))), t(np.zeros((d, 4))))
    assert status_of(e) == _lib.KRCN_ERR_INVALID and "w_cols" in str(e.value)
    Xs = krcn.DeviceCSR(A, n_global=2 * n, shard_mode=_lib.KRCN_SHARD_ROWS)
    V, U = t(np.zeros((d, 2))), t(np.zeros((n, 2)))
    for fn in (lambda: Xs.matvec_block(V), lambda: Xs.rmatvec_block(U), lambda: Xs.hvp_block(w, V)):
        with pytest.raises(_lib.KrcnError) as e:
            fn()
        assert status_of(e) == _lib.KRCN_ERR_UNSUPPORTED


@gpu
def test_no_plan_build_and_the_workspace(mats):
    """Block calls leave a fresh handle's owned bytes larger by the block HVP's
    (n, k) intermediate alone: no pass plans were built.  The intermediate
    grows with k, is one entry of the handle's owner table (which
    krcn_csr_destroy frees) and is not shrunk."""
    A = mats["f1"]
    n, d = A.shape
    fresh = krcn.DeviceCSR(A).owned_bytes()
    X = krcn.DeviceCSR(A)
    w = t(np.ones(n))
    X.matvec_block(t(np.ones((d, 4))))
    X.rmatvec_block(t(np.ones((n, 4))))
    assert X.owned_bytes() == fresh
    X.hvp_block(w, t(np.ones((d, 4))))
    assert X.owned_bytes() - fresh == n * 4 * 8
    X.hvp_block(w, t(np.ones((d, 16))))
    assert X.owned_bytes() - fresh == n * 16 * 8
    X.hvp_block(w, t(np.ones((d, 8))))
    assert X.owned_bytes() - fresh == n * 16 * 8
    X.close()
    assert not X.handle.value


@gpu
def test_matrix_without_nonzeros():
    A = sp.csr_matrix((5, 4), dtype=np.float64)
    X = krcn.DeviceCSR(A)
    V = np.arange(12.0).reshape(4, 3) - 5.0
    l2 = np.array([0.5, 0.0, 2.0])
    assert same_bytes(h(X.matvec_block(t(V))), np.zeros((5, 3)))
    assert same_bytes(h(X.rmatvec_block(t(np.ones((5, 3))))), np.zeros((4, 3)))
    assert np.array_equal(h(X.hvp_block(t(np.ones(5)), t(V), l2=l2)), l2 * V)


# ------------------------------------------------------------ optimizer layer
@gpu
@pytest.mark.parametrize("l2", [0.0, 0.01])
def test_hess_mat_prod_vs_oracle(f1, l2):
    A = golden_csr(f1)
    x = f1["x0"]
    loss = LogisticRegression(A, f1["b"], l2=l2)
    rng = np.random.default_rng(3)
    for kp in (1, 16, 17, 40):
        V = rng.standard_normal((A.shape[1], kp))
        ref = np.stack([O.hess_vec_prod(A, x, V[:, j], l2) for j in range(kp)], axis=1)
        out_np = loss.hess_mat_prod(x, V)
        out_t = loss.hess_mat_prod(x, t(V))
        assert isinstance(out_np, np.ndarray) and out_np.shape == V.shape
        assert isinstance(out_t, torch.Tensor) and out_t.is_cuda and tuple(out_t.shape) == V.shape
        assert same_bytes(out_np, h(out_t))
        for j in range(kp):
            assert rel_err(out_np[:, j], ref[:, j]) < 1e-13, f"k' {kp} column {j}"


@gpu
def test_block_hessian():
    """d = 1030 > KRCN_COORD_MAX and no multiple of the block: hessian(x, block=k)
    against hessian(x), which stays the parent's one HVP per column, bit for bit."""
    rng = np.random.default_rng(11)
    A = sp.random(40, 1030, density=0.05, random_state=rng, format="csr", data_rvs=lambda s: rng.uniform(-1, 1, s))
    assert A.shape[1] > _lib.KRCN_COORD_MAX
    b = np.where(rng.uniform(size=40) < 0.5, -1.0, 1.0)
    x = 0.1 * rng.standard_normal(1030)
    loss = LogisticRegression(A, b, l2=0.01)
    H0 = loss.hessian(x)
    X = loss.device_matrix
    w = X.weights(X.matvec(t(x)))
    e = torch.zeros(1030, dtype=torch.float64, device=DEV)
    cols = []
    for c in range(1030):
        e[c] = 1.0
        cols.append(X.hvp(w, e, l2=0.01))
        e[c] = 0.0
    assert same_bytes(H0, h(torch.stack(cols, dim=1)))
    for k in (8, 16):
        Hk = loss.hessian(x, block=k)
        assert Hk.shape == (1030, 1030)
        print(f"block {k}: vs hessian(x) {rel_err(Hk, H0):.3e}, asymmetry {rel_err(Hk, Hk.T):.3e}")
        assert rel_err(Hk, H0) < 1e-13
        assert rel_err(Hk, Hk.T) < 1e-13
    assert same_bytes(loss.hessian(x), H0)
