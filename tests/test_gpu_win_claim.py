"""Claimed tiles of the window-slices pass (krcn_window.hpp win_stream).

A block's waves take their first three tiles each from a static deal and every
later tile from one LDS counter per block (krcn_geom.hpp win_claim_*), so which
wave runs a tile varies from call to call.  No bit may depend on it: every
(slice, row) partial is summed by one lane (or, past 64 elements, by the wave
in a fixed stripe order) and the combine's order is fixed.

Pass 1 is forced to KRCN_FORMAT_WINDOW; the column count picks the slicing
(krcn_layout.hpp win_slices_mode: the slicing policy does not bear on window
plans): d = 70,001 gives 8 slices x 32 blocks (an fp32 handle: d = 150,001),
d = 1,200,001 gives 85 x 3, d = 3,000,001 gives 256 x 1.  Rows with the same
number of nonzeros in every slice get fixed 64-row tiles cut evenly over a
slice's blocks, so n = 64 x 32 x T rows give every block exactly T tiles.

Every case checks
  * matvec bitwise against a numpy restatement of the documented order: a
    row's products in a slice added left to right from 0 (more than 64 of them:
    64 stripes, element i to stripe i % 64, each left to right, then an xor
    butterfly 32, 16, ..., 1), the slices p, p + 8, ... added left to right
    per phase p < 8, and the tree ((0+1)+(2+3))+((4+5)+(6+7)) over the phases;
  * matvec against scipy's A @ x at the suite's 1e-13 (fp32 handle: 1e-5);
  * matvec byte-identical over 10 calls on one handle.

Cases (the smallest shapes at which the claiming can go wrong):
  1. 2 and 5 tiles a slice under 8 x 32 and 85 x 3: empty segments, fewer tiles
     than waves, every claim past the end;
  2. blocks of exactly 16, 17, 33, 48 and 49 tiles: the static deal alone, a
     second and third static tile for some waves only, no pool, a pool of one;
  3. one block with 422 tiles (27,000 rows, 4 nonzeros a row, one block per
     slice at d = 3,000,001: 256 x 1 — at 2,000 columns a forced window plan
     is an accumulate plan, not a slices plan): a pool of 374 claims;
  4. skewed rows: one row of 700 elements in a slice (its own tile, the
     extra-chunk loop), rows of 65-300 elements a slice (the wave-cooperative
     sum) beside rows of 0-3;
  5. case 2's matrices with fp32 stored values on an fp64 handle and on an
     fp32 handle;
  6. krcn_lanczos, m = 5, on the 49-tile shape: alphas and betas against the
     oracle at the suite's 1e-11, byte-identical over 5 calls.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
import krcn_oracle as O
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
D8, D8_F32, D85, D256 = 70_001, 150_001, 1_200_001, 3_000_001


def t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def per_slice_matrix(n, d, S, per, seed):
    """n rows with exactly `per` nonzeros in every one of the S slices (W = ceil(d / S) columns each)."""
    rng = np.random.default_rng(seed)
    W = -(-d // S)
    width = np.minimum(W, d - W * np.arange(S))            # the last slice is narrower
    stride = width // per                                  # `per` distinct columns: one in each stride-wide cell
    cell = rng.integers(0, stride[None, :, None], size=(n, S, per))
    cols = (np.arange(S) * W)[None, :, None] + np.arange(per)[None, None, :] * stride[None, :, None] + cell
    rows = np.repeat(np.arange(n), S * per)
    vals = rng.uniform(-1, 1, size=rows.size)
    A = sp.csr_matrix((vals, (rows, cols.reshape(-1))), shape=(n, d))
    A.sort_indices()
    assert A.nnz == n * S * per
    return A


def sparse_rows_matrix(n, d, per_row, seed):
    """n rows of `per_row` nonzeros at random columns."""
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(d, size=(n, per_row)), axis=1)
    cols += np.arange(per_row)[None, :]                    # distinct within a row
    cols = np.minimum(cols, d - per_row + np.arange(per_row)[None, :])
    A = sp.csr_matrix((rng.uniform(-1, 1, size=n * per_row), (np.repeat(np.arange(n), per_row), cols.reshape(-1))),
                      shape=(n, d))
    A.sort_indices()
    return A


def skewed_matrix(n, d, S, seed):
    """Rows of 0-3 nonzeros a slice; every 97th row 65-300 in one slice; row 1000 has 700 in slice 2."""
    rng = np.random.default_rng(seed)
    W = -(-d // S)
    rows, cols = [], []
    for r in range(n):
        for s in range(S):
            k = int(rng.integers(0, 4))
            if r % 97 == 5 and s == r % S:
                k = int(rng.integers(65, 301))
            if r == 1000 and s == 2:
                k = 700
            if k:
                rows.append(np.full(k, r))
                cols.append(s * W + np.sort(rng.choice(min(W, d - s * W), size=k, replace=False)))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sp.csr_matrix((rng.uniform(-1, 1, size=rows.size), (rows, cols)), shape=(n, d))
    A.sort_indices()
    return A


def reference_matvec(A, x, S, dtype, values32):
    """The window-slices pass and its combine, restated in numpy with the device's order of additions."""
    n, d = A.shape
    W = -(-d // S)
    ft = np.float64 if dtype == torch.float64 else np.float32
    val = A.data.astype(np.float32 if values32 else ft).astype(ft)
    prod = val * x.astype(ft)[A.indices]
    row = np.repeat(np.arange(n), np.diff(A.indptr))
    key = row.astype(np.int64) * S + A.indices // W          # nondecreasing: (row, slice) runs are contiguous
    start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    length = np.diff(np.r_[start, key.size])
    part = np.zeros((S, n), dtype=ft)
    sums = np.zeros(start.size, dtype=ft)
    short = length <= 64
    for k in range(int(length[short].max(initial=0))):       # left to right, one lane per row
        m = short & (length > k)
        sums[m] = sums[m] + prod[start[m] + k]
    lanes = np.arange(64)
    for g in np.flatnonzero(~short):                         # the whole wave: stripes, then the butterfly
        p = np.zeros(64, dtype=ft)
        e = prod[start[g]:start[g] + length[g]]
        for k in range(0, e.size, 64):
            c = e[k:k + 64]
            p[:c.size] = p[:c.size] + c
        for off in (32, 16, 8, 4, 2, 1):
            p = p + p[lanes ^ off]
        sums[g] = ft(0) + p[0]
    part[(key[start] % S).astype(np.int64), (key[start] // S).astype(np.int64)] = sums
    ph = np.zeros((8, n), dtype=ft)
    for s in range(S):
        ph[s % 8] = ph[s % 8] + part[s]
    return ((ph[0] + ph[1]) + (ph[2] + ph[3])) + ((ph[4] + ph[5]) + (ph[6] + ph[7]))


def handle(A, dtype, values32):
    X = krcn.DeviceCSR(A, dtype=dtype, fmt=krcn.KRCN_FORMAT_WINDOW)
    if values32:
        X.set_value_storage("f32")
    return X


def check_matvec(A, dtype, values32, S, grid, tiles):
    n, d = A.shape
    X = handle(A, dtype, values32)
    assert X.plan_format()["pass1"] == "window-slices"
    s_got, _, t_got, g_got = X.plan_info()["pass1"]
    assert (s_got, g_got, t_got) == (S, grid, tiles), (s_got, g_got, t_got)
    x = np.random.default_rng(11).uniform(-0.5, 0.5, size=d)
    xd = t(x, dtype)
    got = X.matvec(xd).cpu().numpy()
    ref = reference_matvec(A, x, S, dtype, values32)
    Aor = A
    if values32:
        Aor = A.copy()
        Aor.data = Aor.data.astype(np.float32).astype(np.float64)
    e = rel_err(got, Aor @ x)
    print("rows differing from the restated order:", int((got != ref).sum()), "rel_err vs scipy", e)
    np.testing.assert_array_equal(got, ref)
    assert e < (1e-13 if dtype == torch.float64 else 1e-5)
    raw = got.tobytes()
    for _ in range(10):
        assert X.matvec(xd).cpu().numpy().tobytes() == raw
    return X


@functools.lru_cache(maxsize=None)
def block_tiles_matrix(T, d):
    return per_slice_matrix(64 * 32 * T, d, 8, 2, seed=T)


@pytest.mark.parametrize("d,S,grid", [(D8, 8, 256), (D85, 85, 255)])
@pytest.mark.parametrize("n", [128, 300])
def test_few_tiles(n, d, S, grid):
    check_matvec(sparse_rows_matrix(n, d, 16, seed=n), torch.float64, False, S, grid, -(-n // 64))


@pytest.mark.parametrize("T", [16, 17, 33, 48, 49])
def test_tiles_per_block(T):
    check_matvec(block_tiles_matrix(T, D8), torch.float64, False, 8, 256, 32 * T)


def test_long_block():
    check_matvec(sparse_rows_matrix(27_000, D256, 4, seed=3), torch.float64, False, 256, 256, 422)


def test_skewed_rows():
    A = skewed_matrix(4096, D8, 8, seed=5)
    per = np.diff(A.indptr)
    assert per.max() >= 700
    check_matvec(A, torch.float64, False, 8, 256, 64)


@pytest.mark.parametrize("T", [16, 17, 33, 48, 49])
def test_tiles_per_block_values32(T):
    X = check_matvec(block_tiles_matrix(T, D8), torch.float64, True, 8, 256, 32 * T)
    assert X.plan_value_bytes()["pass1"] == 4


@pytest.mark.parametrize("T", [16, 17, 33, 48, 49])
def test_tiles_per_block_f32(T):
    check_matvec(block_tiles_matrix(T, D8_F32), torch.float32, False, 8, 256, 32 * T)


def test_lanczos_49_tiles():
    A = block_tiles_matrix(49, D8)
    n, d = A.shape
    X = handle(A, torch.float64, False)
    assert X.plan_format()["pass1"] == "window-slices"
    rng = np.random.default_rng(13)
    x = rng.uniform(-0.2, 0.2, size=d)
    b = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    Ax = X.matvec(t(x, torch.float64))
    wd = X.weights(Ax)
    g = X.gradient(Ax, t(O.labels01(b), torch.float64))
    wh, gh = wd.cpu().numpy(), g.cpu().numpy()
    _, al_r, be_r, _ = O.lanczos(lambda q: O.hvp_from_weights(A, wh, q), gh, 5)
    raw = None
    for _ in range(5):
        V, al, be, info = X.lanczos(wd, g, 5)
        assert info.m_eff == 5 and not info.breakdown
        al, be = np.asarray(al), np.asarray(be)
        now = (al.tobytes(), be.tobytes(), V.cpu().numpy().tobytes())
        assert raw is None or now == raw
        raw = now
    ea, eb = rel_err(al, al_r), rel_err(be, be_r)
    print("lanczos m = 5: alphas", ea, "betas", eb)
    assert ea < 1e-11 and eb < 1e-11
