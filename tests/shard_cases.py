"""Case builders of the rank-edge tests (tests/test_shard_cases.py checks them
on the CPU, tests/test_gpu_rank_edges.py runs them on virtual ranks).

`crafted` builds a matrix whose nnz-balanced partition (krcn.dist.plan) is a
chosen list of block sizes, so a test can put a rank on 1, 255, 256 or 257
rows or columns: the sizes where the vector grids, the row-apply grids and the
packed tails of the sharded Lanczos all-reduces meet a workgroup boundary.

How the cut lands where it should: every block holds the same nonzero total
T = 2 max(sizes), so the running sum of the row lengths equals k T exactly at
the end of block k, and because every row is non-empty (T >= 2 s for every
block size s) it is below k T everywhere before.  balanced_ranges cuts at the
first index whose running sum reaches k total / parts = k T.
"""
import numpy as np
import scipy.sparse as sp

from krcn import dist as kdist

# the partitions of the edge cases: block sizes in rank order
EDGE_SIZES = [
    (1, 256, 257),
    (255, 1, 256),
    (257, 256, 255, 1),
    (256, 257),
    (1, 1),
    (1,) * 8,
    (33, 1, 64, 65, 63, 2, 128, 31),
]
OTHER = 600   # the uncut dimension of every crafted case (>= T = 514: a one-row block fits)


def size_id(sizes):
    return "x".join(str(s) for s in sizes)


def crafted(sizes, other, seed, integer=False):
    """CSR matrix of sum(sizes) rows and `other` columns whose rows-partition
    over len(sizes) ranks is exactly `sizes` (its transpose: the same
    cols-partition).  Block k holds T = 2 max(sizes) nonzeros spread over its
    rows as floor(T / s) or ceil(T / s), sorted distinct columns per row (every
    row has at least two entries; a block's first row always holds columns 0
    and other - 1).
    integer=True draws the values from {-3..3} without 0 (a stored zero would
    not survive every sparse conversion), so every sum of products with
    integer vectors is an exact small integer; else uniform on (-1, 1) over the
    square root of the row's length.  That scaling gives every row a norm of
    the same order: with plain uniform values the one row of a one-row block
    (514 entries beside rows of 2) is an isolated top eigenvalue of
    X^T D X / n, Lanczos converges to it within a few steps and then amplifies
    rounding by 1e4 a step — the oracle's own alphas at m = 10 move by 2e-2
    under a 1e-16 perturbation of the HVP, against 5e-16 with the scaling
    (tests/test_shard_cases.py)."""
    rng = np.random.default_rng(seed)
    T = 2 * max(sizes)
    if T > other:
        raise ValueError(f"a block of one row needs {T} columns, got {other}")
    lens = []
    for s in sizes:
        q, r = divmod(T, s)
        blk = np.full(s, q, dtype=np.int64)
        blk[:r] += 1
        lens.append(blk)
    lens = np.concatenate(lens)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    firsts = set(np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist())

    def columns(i, k):
        # a block's first row holds the first and the last column, so both ends of the uncut dimension
        # receive a term from every rank: a sum over ranks that drops its tail element changes a result
        if i in firsts:
            return np.sort(np.concatenate([[0, other - 1], 1 + rng.choice(other - 2, k - 2, replace=False)]))
        return np.sort(rng.choice(other, k, replace=False))

    indices = np.concatenate([columns(i, int(k)) for i, k in enumerate(lens)]).astype(np.int32)
    if integer:
        data = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=int(indptr[-1]))
    else:
        data = rng.uniform(-1.0, 1.0, int(indptr[-1])) / np.sqrt(np.repeat(lens, lens))
    return sp.csr_matrix((data, indices, indptr), shape=(len(lens), other))


def crafted_case(sizes, mode, seed, integer=False):
    """The crafted matrix cut by `mode` ("rows" or "cols") into `sizes`."""
    A = crafted(sizes, OTHER, seed, integer)
    if mode == "cols":
        A = A.T.tocsr()
        A.sort_indices()
    return A


def labels(n, seed):
    """n labels in {-1, 1} with both classes present whenever n >= 2."""
    rng = np.random.default_rng(seed)
    b = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if n >= 2:
        b[0], b[-1] = -1.0, 1.0
    return b


def integer_vector(n, lo, hi, seed, nonzero=False, ends=None):
    """n integers of [lo, hi] as float64; nonzero=True leaves 0 out, `ends`
    sets the first and the last entry (the elements at the edge of a grid or
    of an all-reduce must not be multiplied away)."""
    vals = np.array([k for k in range(lo, hi + 1) if k != 0 or not nonzero], dtype=np.float64)
    v = np.random.default_rng(seed).choice(vals, n)
    if ends is not None:
        v[0] = v[-1] = float(ends)
    return v


def integer_inputs(n, d):
    """(x, v, u, w) of the exact layout check: x, v (d) and u (n) from
    {-3..3} without 0, the weights w (n) from {0..4} with w[0] = w[-1] = 4."""
    return (integer_vector(d, -3, 3, 1, nonzero=True), integer_vector(d, -3, 3, 2, nonzero=True),
            integer_vector(n, -3, 3, 3, nonzero=True), integer_vector(n, 0, 4, 4, ends=4))


def block_nnz(A, world, mode):
    """(bounds, [nonzeros of rank r's block]) of the `mode` partition over `world` ranks."""
    m, bounds = kdist.plan(A, world, mode)
    return bounds, [int(kdist.extract(A, m, bounds, r).nnz) for r in range(world)]


def ordered_matvec(A, v, dtype, reverse):
    """A v with every row's products added one at a time in `dtype`, in CSR
    order or (reverse) from the row's last entry to its first."""
    A = sp.csr_matrix(A)
    dt = np.dtype(dtype).type
    out = np.zeros(A.shape[0], dtype=dtype)
    for i in range(A.shape[0]):
        ks = range(A.indptr[i], A.indptr[i + 1])
        acc = dt(0)
        for k in (reversed(ks) if reverse else ks):
            acc = dt(acc + dt(dt(A.data[k]) * dt(v[A.indices[k]])))
        out[i] = acc
    return out


def integer_magnitude(A, x, u, v, w):
    """The largest absolute partial sum any summation order can meet in
    X x, X^T u and X^T (w * X v): the same products with every factor replaced
    by its absolute value."""
    Aa = abs(sp.csr_matrix(A))
    t = Aa @ np.abs(v)
    return float(max((Aa @ np.abs(x)).max(), (Aa.T @ np.abs(u)).max(), (Aa.T @ (np.abs(w) * t)).max()))
