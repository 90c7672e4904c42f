"""krcn_hessian_gram on the GPU: the dense Hessian X^T diag(w) X / n + l2 I as one
Gram product over the dense X^T image, on v_mfma_f64_16x16x4_f64.

1. Exact data (small integers): every sum is an exact integer, so any order
   gives the same bytes and H must be byte-equal to numpy's for every split.
   This is the layout check: a wrong row map, a swapped mirror or an unwritten
   tile cannot pass (H is NaN before the call).
2. The bound.  With u = 2^-53 and S_ab = sum_r |x_ra w_r x_rb| / n,
       |H_ab - Href_ab| <= (n + 4) u (S_ab + l2 [a == b]):
   one rounding in x w, at most n - 1 in the sum (any order, fused
   multiply-adds), one in the division, one in + l2.  Derived, not measured.
   Href is the longdouble value of (A.T * w) @ A / n + l2 I.  Where the bound
   is 0 the entry must be exactly 0.  The largest ratio error / bound is
   printed (numpy's own fp64 product stays below 0.27 on these shapes).
3. Refusals, 4. the Python layer, 5. Cubic_LS(gram_hessian=True).

The shapes are the smallest at which the tiling can go wrong: T and KS (the tile
edge and the slab of the summed index) come from krcn.gram_geometry.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
from krcn import _lib
from optimizer.cubic import Cubic_LS
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu

DEV = "cuda"
DENSE = 5
U = 2.0 ** -53
G0 = krcn.gram_geometry(1, 1)
T, KS = G0["T"], G0["KS"]
KINDS = ("f64", "f64-values-f32", "f32")


def t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def host(x):
    torch.cuda.synchronize()
    return x.cpu().numpy()


def handle(A, kind):
    """A dense-format handle of one of the three stored kinds, its images built, and the matrix it computes with."""
    A = sp.csr_matrix(A)
    if kind == "f32":
        X = krcn.DeviceCSR(A, dtype=torch.float32, fmt=DENSE)
    else:
        X = krcn.DeviceCSR(A, fmt=DENSE, values="f32" if kind == "f64-values-f32" else 0)
    X.plan_info()
    assert X.plan_format()["pass2"] == "dense"
    assert X.plan_value_bytes()["pass2"] == (8 if kind == "f64" else 4)
    Aeff = A.toarray() if kind == "f64" else A.toarray().astype(np.float32).astype(np.float64)
    return X, Aeff


def gram(X, w, l2, split):
    """hessian_gram into a NaN-filled H under a forced split (0: the rule)."""
    X.set_gram_split(split)
    H = torch.full((X.d, X.d), float("nan"), dtype=torch.float64, device=DEV)
    out = X.hessian_gram(t(w, X.dtype), l2=l2, out=H)
    assert out is H
    return host(H)


def bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 1. exact data
EXACT_SHAPES = [(5, 17), (67, T + 1), (130, 2 * T + 3), (3 * KS + 2, T - 1)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d", EXACT_SHAPES)
def test_exact_integers_every_split(n, d, kind):
    rng = np.random.default_rng(1000 * n + d)
    Xi = rng.integers(-3, 4, size=(n, d)).astype(np.float64) * (rng.random((n, d)) < 0.7)
    wi = rng.integers(0, 5, size=n).astype(np.float64)
    want = (Xi.T * wi) @ Xi / n + 0.5 * np.eye(d)
    # (order-independent on such data: every partial sum is an integer below 2^53)
    assert bytes_equal(want, (Xi[::-1].T * wi[::-1]) @ Xi[::-1] / n + 0.5 * np.eye(d))
    X, Aeff = handle(Xi, kind)
    assert np.array_equal(Aeff, Xi)
    slabs = krcn.gram_geometry(d, n)["slabs"]
    for split in (1, 2, 3, 7, slabs + 1):
        got = gram(X, wi, 0.5, split)
        bad = np.argwhere(~((got == want) & np.isfinite(got)))
        assert bad.size == 0, f"split {split}: {len(bad)} entries differ, first at {bad[0]}: " \
                              f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        assert bytes_equal(got, want), f"split {split}"
    X.close()


# ---------------------------------------------------------------- 2. the bound
BOUND_SHAPES = [(1, 1), (3, 1), (4, 16), (5, 17), (KS - 1, 15), (KS, T), (KS + 1, T + 1), (3 * KS + 2, 2 * T + 3)]


def bound_problem(n, d, kind):
    rng = np.random.default_rng(77 * n + d)
    A = rng.standard_normal((n, d)) * (rng.random((n, d)) < 0.7)
    if d >= 2:
        A[:, d // 2] = 0.0                  # one empty column: its row and column of H are exactly l2 [a == b]
    w = rng.random(n) * 0.25
    if n >= 3:
        w[rng.integers(0, n, size=max(1, n // 5))] = 0.0
    if kind == "f32":
        w = w.astype(np.float32).astype(np.float64)    # what the fp32 handle is given, widened
    return A, w


def reference(Aeff, w, l2):
    """(Href, bound) in longdouble: the value, and (n + 4) u (S + l2 I)."""
    n, d = Aeff.shape
    Al, wl = Aeff.astype(np.longdouble), w.astype(np.longdouble)
    eye = np.eye(d, dtype=np.longdouble)
    Href = (Al.T * wl) @ Al / n + np.longdouble(l2) * eye
    S = (np.abs(Al).T * np.abs(wl)) @ np.abs(Al) / n
    return Href, (n + 4) * np.longdouble(U) * (S + np.longdouble(l2) * eye)


def worst_ratio(H, Href, bound):
    err = np.abs(H.astype(np.longdouble) - Href)
    zero = bound == 0
    assert np.all(H[zero] == 0.0), "an entry whose bound is 0 must be exactly 0"
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d", BOUND_SHAPES)
def test_error_bound(n, d, kind):
    A, w = bound_problem(n, d, kind)
    X, Aeff = handle(A, kind)
    worst = 0.0
    for l2 in (0.0, 0.01):
        Href, bound = reference(Aeff, w, l2)
        numpy_ratio = worst_ratio((Aeff.T * w) @ Aeff / n + l2 * np.eye(d), Href, bound)
        for split in (0, 3):
            H = gram(X, w, l2, split)
            assert np.isfinite(H).all()
            ratio = worst_ratio(H, Href, bound)
            print(f"n {n} d {d} {kind} l2 {l2} split {split}: error / bound {ratio:.3f} (numpy {numpy_ratio:.3f})")
            worst = max(worst, ratio)
            assert bytes_equal(H, H.T.copy()), "H is exactly symmetric"
            assert bytes_equal(H, gram(X, w, l2, split)), "two calls return the same bytes"
            assert ratio <= 1.0, f"l2 {l2} split {split}: error / bound = {ratio}"
    print(f"n {n} d {d} {kind}: largest error / bound {worst:.3f}")
    X.close()


# ---------------------------------------------------------------- 3. refusals
def small_problem(n=20, d=9, seed=5):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, d)) * (rng.random((n, d)) < 0.7)
    return A, rng.random(n) * 0.25


def test_pass2_not_dense_is_unsupported():
    A, w = small_problem()
    X = krcn.DeviceCSR(sp.csr_matrix(A), fmt=1)
    with pytest.raises(krcn.KrcnError) as e:
        X.hessian_gram(t(w))
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    assert "krcn_csr_set_pass_format(h, 2, KRCN_FORMAT_DENSE)" in str(e.value)
    # a dense pass 1 alone does not help
    X.set_pass_format(1, DENSE)
    with pytest.raises(krcn.KrcnError) as e:
        X.hessian_gram(t(w))
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    X.close()


def test_pass1_sparse_pass2_dense_works():
    A, w = small_problem()
    X = krcn.DeviceCSR(sp.csr_matrix(A), fmt=1, pass_formats=(-1, DENSE))
    assert X.plan_format() == {"pass1": "wave", "pass2": "dense"}
    Href, bound = reference(A, w, 0.01)
    assert worst_ratio(gram(X, w, 0.01, 0), Href, bound) <= 1.0
    X.close()


@pytest.mark.parametrize("n,d", [(7, 5), (0, 3)])
def test_no_nonzeros_is_l2_identity(n, d):
    X = krcn.DeviceCSR(sp.csr_matrix((n, d), dtype=np.float64), fmt=DENSE)
    w = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    H = torch.full((d, d), float("nan"), dtype=torch.float64, device=DEV)
    X.hessian_gram(w, l2=0.25, out=H)
    assert bytes_equal(host(H), 0.25 * np.eye(d))
    X.close()


def test_workspace_is_owned_and_grows_on_demand():
    A, w = small_problem(n=3 * KS + 2, d=T + 1)
    X, _ = handle(A, "f64")
    gram(X, w, 0.0, 1)
    base = X.owned_bytes()                      # split 1 allocates nothing
    gram(X, w, 0.0, 2)
    tile = T * T * 8
    assert X.owned_bytes() == base + krcn.gram_geometry(T + 1, 3 * KS + 2, 2)["ws_bytes"] == base + 3 * 2 * tile
    gram(X, w, 0.0, 7)
    assert X.owned_bytes() == base + 3 * 7 * tile
    gram(X, w, 0.0, 3)                          # fits: nothing changes
    assert X.owned_bytes() == base + 3 * 7 * tile
    X.close()


# ---------------------------------------------------------------- 4. the Python layer
@pytest.mark.parametrize("d", [40, 1030])
def test_loss_hessian_gram_vs_default(d):
    n = 48
    rng = np.random.default_rng(d)
    A = rng.standard_normal((n, d)) * (rng.random((n, d)) < 0.7)
    b = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    x = 0.3 * rng.standard_normal(d)
    loss = LogisticRegression(sp.csr_matrix(A), b, l1=0, l2=0.05, format="dense")
    H0 = loss.hessian(x)
    Hg = loss.hessian(x, gram=True)
    assert Hg.shape == (d, d) and Hg.dtype == np.float64 and bytes_equal(Hg, Hg.T.copy())
    w = host(loss._weights_for(x))
    _, bound = reference(A, w, 0.05)
    # both sides satisfy the bound around the exact value
    assert np.all(np.abs(Hg.astype(np.longdouble) - H0.astype(np.longdouble)) <= 2 * bound)
    assert bytes_equal(loss.hessian(x), H0), "the default path is untouched by a Gram call"
    with pytest.raises(ValueError):
        loss.hessian(x, block=4, gram=True)


def test_loss_hessian_gram_needs_a_dense_image():
    A, _ = small_problem()
    b = np.where(np.arange(A.shape[0]) % 2 == 0, 1.0, -1.0)
    loss = LogisticRegression(sp.csr_matrix(A), b, l1=0, l2=0.0, format=1)
    with pytest.raises(krcn.KrcnError) as e:
        loss.hessian(np.zeros(A.shape[1]), gram=True)
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED


# ---------------------------------------------------------------- 5. Cubic_LS
def test_cubic_ls_gram_hessian_matches_the_default():
    """A plumbing check: the tolerance is eight orders above the Hessians'
    difference, and l2 = 0.1 keeps the subproblem well conditioned."""
    n, d = 80, 24
    rng = np.random.default_rng(80)
    A = rng.standard_normal((n, d)) * (rng.random((n, d)) < 0.7)
    b = np.where(A @ rng.standard_normal(d) >= 0, 1.0, -1.0)
    x0 = np.full(d, 0.5)
    xs = []
    for gram_hessian in (False, True):
        loss = LogisticRegression(sp.csr_matrix(A), b, l1=0, l2=0.1, format="dense")
        opt = Cubic_LS(loss=loss, reg_coef=1e-2, cubic_solver="full", label="full", tqdm=False,
                       gram_hessian=gram_hessian)
        opt.run(x0=x0, it_max=3)
        xs.append([np.asarray(v, dtype=np.float64) for v in opt.trace.xs])
    assert len(xs[0]) == len(xs[1]) == 4
    for a, g in zip(*xs):
        assert np.abs(a - g).max() <= 1e-8 * np.abs(a).max()
    assert np.abs(xs[0][-1] - x0).max() > 1e-3      # the steps moved
