"""Data-cut tiles of window-slices plans (krcn_layout.hpp win_layout, krcn_window.hpp).

A long pass-1 stream of short rows (the fixed rule would take 16- or 32-row
tiles, and a slice's blocks get 48 tiles each or more) cuts every slice's
tiles from the data: as many rows, up to 64, as fill one 256-nonzero chunk.
The shapes are the smallest that engage it: n = 50,000 rows at 8 slices x 32
blocks give 1563 >= 32 x 48 fixed tiles of 32 rows, at about 5 nonzeros per
row and slice (2 M nonzeros).  Forced KRCN_FORMAT_WINDOW; fp64 at d = 70,001
(uniform and skewed rows), the same under fp32 value storage, an fp32 handle
at d = 150,001, and edge patterns written into the uniform matrix: more than
64 consecutive empty rows in a slice, an entirely empty slice, rows of 300 and
700 nonzeros in one slice, and a tile that fills its chunk exactly from a
misaligned start.

Every case asserts that
  * plan_info reports fewer tiles than ceil(n / 32): the data-cut path ran;
  * matvec is bitwise the concatenation of matvec over row-block sub-handles
    of 12,500 rows at the same d, which keep fixed tiles (asserted): slice
    cuts and combine order depend on d and S only, a row's slice sum is a
    function of the row alone;
  * hvp agrees with the oracle at 1e-13 (fp32 handle: 1e-5, the suite's fp32
    HVP bound; fp32 values: the oracle over the rounded matrix);
  * lanczos at m = 10, l2 = 0 and 0.01, gives the oracle's alphas / betas at
    1e-11 (test_lanczos_early_alpha_l2's).  The fp32 handle: 1e-4 — fp32
    arithmetic cannot hold 1e-11; each HVP is good to 1e-5 (above), an alpha
    is one HVP's Rayleigh quotient and a beta one norm, and ten steps of the
    recurrence compound at most linearly on this well-spread spectrum.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
import krcn_oracle as O
from conftest import rel_err
from krcn import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, NNZ, BLOCK = 50_000, 2_000_000, 12_500


def t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def with_edges(A):
    """The edge patterns, in slices of W = ceil(d / 8) columns."""
    n, d = A.shape
    W = -(-d // 8)
    C = A.tocoo()
    r, c, v = C.row, C.col, C.data
    sl = c // W
    keep = ~((sl == 3) |                                   # an entirely empty slice
             ((sl == 1) & (r >= 1000) & (r < 1101)) |      # 101 consecutive empty rows
             ((sl == 0) & (r < 4)) | ((sl == 2) & (r == 5000)) | ((sl == 4) & (r == n - 1)))
    rows, cols = [r[keep]], [c[keep]]
    # slice 0 begins at element 0: row 0 alone (250; one more row would pass 256), then rows 1-2 from element
    # 250 (250 % 4 = 2) with 7 + 247 = 254 nonzeros — 2 + 254 = 256 exactly; rows past a chunk in slices 2 and 4
    for row, s, k in ((0, 0, 250), (1, 0, 7), (2, 0, 247), (3, 0, 1), (5000, 2, 300), (n - 1, 4, 700)):
        rows.append(np.full(k, row))
        cols.append(s * W + 3 * np.arange(k))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.concatenate([v[keep], np.random.default_rng(2).uniform(-1, 1, size=len(rows) - int(keep.sum()))])
    B = sp.csr_matrix((vals, (rows, cols)), shape=(n, d))
    B.sort_indices()
    return B


@functools.lru_cache(maxsize=None)
def problem(d, kind):
    A, b = synth.make_problem(None, n=N, d=d, nnz=NNZ, skew=kind == "skew")
    if kind == "edges":
        A = with_edges(A)
    return A, b


CASES = {
    "f64-uniform": (70_001, "uniform", torch.float64, 0),
    "f64-skew": (70_001, "skew", torch.float64, 0),
    "f64-uniform-values32": (70_001, "uniform", torch.float64, 1),
    "f64-skew-values32": (70_001, "skew", torch.float64, 1),
    "f32-uniform": (150_001, "uniform", torch.float32, 0),
    "f64-edges": (70_001, "edges", torch.float64, 0),
}


def handle(A, dtype, values):
    X = krcn.DeviceCSR(A, dtype=dtype, fmt=krcn.KRCN_FORMAT_WINDOW)
    if values:
        X.set_value_storage("f32")
        assert X.plan_value_bytes() == {"pass1": 4, "pass2": 4}
    return X


@pytest.mark.parametrize("case", sorted(CASES))
def test_data_cut_tiles(case):
    d, kind, dtype, values = CASES[case]
    A, b = problem(d, kind)
    n = A.shape[0]
    X = handle(A, dtype, values)
    assert X.plan_format()["pass1"] == "window-slices"
    S, _, tiles, grid = X.plan_info()["pass1"]
    print(case, "pass1 plan", (S, tiles, grid))
    assert (S, grid) == (8, 256)
    assert tiles < -(-n // 32)            # the data-cut path ran
    Aor = A
    if values:                            # the oracle over the matrix the plans hold
        Aor = A.copy()
        Aor.data = Aor.data.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.2, 0.2, size=d)
    v = rng.standard_normal(d)
    tol = 1e-13 if dtype == torch.float64 else 1e-5

    # matvec: bitwise the fixed-tile sub-handles'
    Ax = X.matvec(t(x, dtype))
    parts = []
    for r0 in range(0, n, BLOCK):
        sub = handle(A[r0:r0 + BLOCK], dtype, values)
        assert sub.plan_format()["pass1"] == "window-slices"
        s_sub, _, t_sub, _ = sub.plan_info()["pass1"]
        rows = min(BLOCK, n - r0)
        assert s_sub == 8 and t_sub in {-(-rows // R) for R in (16, 32, 64)}   # fixed tiles
        parts.append(sub.matvec(t(x, dtype)).cpu().numpy())
        del sub
    got = Ax.cpu().numpy()
    ref = np.concatenate(parts)
    print(case, "matvec rows differing from the sub-handles:", int((got != ref).sum()),
          "rel_err vs scipy", rel_err(got, Aor @ x))
    np.testing.assert_array_equal(got, ref)

    # hvp against the oracle
    w = O.hessian_weights(Aor, x)
    y = X.hvp(t(w, dtype), t(v, dtype)).cpu().numpy()
    e = rel_err(y, O.hvp_from_weights(Aor, w, v))
    print(case, "hvp rel_err", e)
    assert e < tol

    # lanczos against the oracle, from the device's own weights and gradient
    wd = X.weights(Ax)
    g = X.gradient(Ax, t(O.labels01(b), dtype))
    wh, gh = wd.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    ltol = 1e-11 if dtype == torch.float64 else 1e-4
    for l2 in (0.0, 0.01):
        V, al, be, info = X.lanczos(wd, g, 10, l2=l2)
        _, al_r, be_r, _ = O.lanczos(lambda q: O.hvp_from_weights(Aor, wh, q, l2=l2), gh, 10)
        ea, eb = rel_err(al, al_r), rel_err(be, be_r)
        print(case, "lanczos l2 =", l2, "alphas", ea, "betas", eb)
        assert info.m_eff == 10 and not info.breakdown
        assert ea < ltol and eb < ltol
