"""Every element counted once: the fixed-order reductions (block_sum,
sum_partials, k_reduce2, k_finish behind krcn_loss_mean / krcn_dot /
krcn_diff_norm) and the element-wise k_weights at lengths around a wave (64),
a block (256), the 1024-block cap of vec_grid (256 x 1024 = 262144, past which
the grid-stride loop takes a second, third and fourth trip) and their
neighbours.

The inputs make every sum an integer below 2^53, exact in any order, so a
dropped, repeated or out-of-range element changes the result and the
comparisons need no tolerance.  Vectors live inside larger allocations whose
neighbouring elements hold values that would swamp the sum (inputs) or a
canary that must survive (outputs).
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
from krcn import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 256 * 1024
L = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, CAP - 1, CAP, CAP + 1, CAP + 257, 3 * CAP + 1]
DTYPES = {"fp64": (np.float64, torch.float64, 1e300), "fp32": (np.float32, torch.float32, 1e30)}
GUARD = 16


def inside(a, tdt, fill):
    """`a` on the device as a view of a larger buffer with GUARD elements of `fill` on both sides."""
    buf = torch.full((len(a) + 2 * GUARD,), fill, dtype=tdt, device=DEV)
    v = buf[GUARD:GUARD + len(a)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV, tdt))
    assert v.is_contiguous()
    return buf, v


@pytest.fixture(scope="module", params=list(DTYPES), ids=list(DTYPES))
def handles(request):
    """Per dtype, built on demand and kept: n x 1 handles (one nonzero per row) for
    the N space, 1 x d handles for the D space."""
    npdt, tdt, big = DTYPES[request.param]
    made = {}

    def get(space, ln):
        if (space, ln) not in made:
            if space == "n":
                A = sp.csr_matrix((np.ones(ln), np.zeros(ln, dtype=np.int32), np.arange(ln + 1, dtype=np.int32)), shape=(ln, 1))
            else:
                A = sp.csr_matrix((np.ones(1), np.zeros(1, dtype=np.int32), np.array([0, 1], dtype=np.int32)), shape=(1, ln))
            made[(space, ln)] = krcn.DeviceCSR(A, dtype=tdt)
        return made[(space, ln)]

    yield npdt, tdt, big, get
    for X in made.values():
        X.close()


# --------------------------------------------------------------------- loss
def test_loss_mean_counts_every_row_once(handles):
    """b = 1 and Ax_i = -(64 + i % 1021) < -33: the term is -logsig(Ax_i) = -Ax_i, an integer."""
    npdt, tdt, big, get = handles
    for n in L:
        X = get("n", n)
        i = np.arange(n, dtype=np.int64)
        terms = 64 + i % 1021
        want = float(int(terms.sum())) / n
        Ax = (-terms).astype(npdt)
        plain = X.loss_mean(torch.from_numpy(Ax).to(DEV), torch.ones(n, dtype=tdt, device=DEV))
        assert plain == want, f"n = {n}: {plain!r} != {want!r}"
        # a neighbour read as a row would add (1 - 0) * big - logsig(big) = big
        _, Axv = inside(Ax, tdt, big)
        _, bv = inside(np.ones(n, dtype=npdt), tdt, 0.0)
        canary = X.loss_mean(Axv, bv)
        assert canary == want, f"n = {n} inside a larger buffer: {canary!r} != {want!r}"


# -------------------------------------------------------- dot and diff_norm
@pytest.mark.parametrize("space", ["n", "d"])
def test_dot_and_diff_norm_count_every_element_once(handles, space):
    npdt, tdt, big, get = handles
    code = _lib.KRCN_SPACE_N if space == "n" else _lib.KRCN_SPACE_D
    rng = np.random.default_rng(17)
    for ln in L:
        X = get(space, ln)
        a = rng.integers(-3, 4, ln)
        b = rng.integers(-3, 4, ln)
        a[-1], b[-1] = 3, -3                     # the tail element always counts
        _, av = inside(a.astype(npdt), tdt, big)
        _, bv = inside(b.astype(npdt), tdt, big)
        dot = int((a * b).sum())
        assert X.dot(av, bv, space=code) == float(dot), f"{space} space, length {ln}"
        assert X.diff_norm(av, bv, space=code) == math.sqrt(int(((a - b) ** 2).sum())), f"{space} space, length {ln}"
        assert X.diff_norm(av, space=code) == math.sqrt(int((a * a).sum())), f"{space} space, length {ln}"


# ------------------------------------------------------------- element-wise
def test_weights_at_every_index_and_nowhere_else(handles):
    """Three margins cycling with the index: w_i is the n = 1 result of Ax_i at
    every i, and the GUARD elements on both sides of the output keep their canary."""
    npdt, tdt, big, get = handles
    vals = np.array([-2.5, 0.75, 9.0], dtype=npdt)      # expit(9) is still below 1 in fp32
    one = get("n", 1)
    w1 = torch.cat([one.weights(torch.from_numpy(vals[k:k + 1]).to(DEV)) for k in range(3)])
    assert len(set(w1.tolist())) == 3 and (w1 > 0).all()
    canary = -7.0
    for n in L:
        X = get("n", n)
        idx = torch.arange(n, device=DEV) % 3
        _, Axv = inside(vals[np.arange(n) % 3], tdt, float("nan"))
        buf, out = inside(np.full(n, canary, dtype=npdt), tdt, canary)
        got = X.weights(Axv, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out, w1[idx]), f"n = {n}"
        assert (buf[:GUARD] == canary).all() and (buf[GUARD + n:] == canary).all(), f"n = {n}: wrote outside the output"
