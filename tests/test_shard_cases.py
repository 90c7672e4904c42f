"""The case builders of the rank-edge tests, checked on the CPU.

tests/test_gpu_rank_edges.py relies on three facts about its inputs that the
GPU cannot tell it: the crafted matrices are cut by krcn.dist.plan exactly
where they were built to be cut, the integer variants make every sum exact
whatever its order, and the column cuts of the breakdown fixtures hand some
ranks a block without a single nonzero.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import krcn_oracle as O
import shard_cases as SC
from conftest import golden_csr, rel_err
from krcn import dist as kdist


@pytest.mark.parametrize("mode", ["rows", "cols"])
@pytest.mark.parametrize("integer", [False, True], ids=["real", "integer"])
@pytest.mark.parametrize("sizes", SC.EDGE_SIZES, ids=SC.size_id)
def test_crafted_partition_is_the_wanted_one(sizes, integer, mode):
    A = SC.crafted_case(sizes, mode, seed=11, integer=integer)
    cut, other = (A.shape[0], A.shape[1]) if mode == "rows" else (A.shape[1], A.shape[0])
    assert (cut, other) == (sum(sizes), SC.OTHER)
    got_mode, bounds = kdist.plan(A, len(sizes), mode)
    assert got_mode == mode
    np.testing.assert_array_equal(np.diff(bounds), sizes)
    # no row holds more entries than there are columns, no column more than rows
    assert np.diff(A.indptr).max() <= A.shape[1]
    assert np.bincount(A.indices, minlength=A.shape[1]).max() <= A.shape[0]
    # sorted distinct columns in every row, no stored zero, every rank's block holds T nonzeros
    assert A.has_sorted_indices and all(np.all(np.diff(A.indices[a:b]) > 0) for a, b in zip(A.indptr, A.indptr[1:]))
    assert np.all(A.data != 0)
    _, nnz = SC.block_nnz(A, len(sizes), mode)
    assert nnz == [2 * max(sizes)] * len(sizes)
    # the blocks side by side are the matrix
    blocks = [kdist.extract(A, mode, bounds, r) for r in range(len(sizes))]
    whole = sp.vstack(blocks) if mode == "rows" else sp.hstack(blocks)
    assert (whole != A).nnz == 0


@pytest.mark.parametrize("mode", ["rows", "cols"])
@pytest.mark.parametrize("sizes", SC.EDGE_SIZES, ids=SC.size_id)
def test_integer_variant_sums_exactly_in_any_order(sizes, mode):
    """X x, X^T u and X^T (w * X v) of the integer variant with the vectors the
    GPU test uses: every product and every partial sum is an integer below
    2^24 in magnitude (so exact in fp32 and fp64 alike, in any order), and a
    reversed summation gives the same bytes."""
    A = SC.crafted_case(sizes, mode, seed=11, integer=True)
    n, d = A.shape
    x, v, u, w = SC.integer_inputs(n, d)
    assert set(np.unique(A.data)) <= {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert SC.integer_magnitude(A, x, u, v, w) < 2 ** 24
    assert np.all(x != 0) and np.all(v != 0) and np.all(u != 0) and w[0] == w[-1] == 4 and w.min() >= 0
    # both ends of the uncut dimension get a nonzero term from every rank's block
    mode_, bounds = kdist.plan(A, len(sizes), mode)
    for r in range(len(sizes)):
        B = kdist.extract(A, mode_, bounds, r).tocsc()
        ends = B[:, [0, -1]] if mode == "rows" else B.T.tocsc()[:, [0, -1]]
        assert np.all(np.diff(ends.indptr) >= 1), (mode, r)
    for dtype in (np.float64, np.float32):
        for M, vec in ((A, x), (A.T.tocsr(), u), (A.T.tocsr(), w * (A @ v))):
            fwd = SC.ordered_matvec(M, vec, dtype, reverse=False)
            bwd = SC.ordered_matvec(M, vec, dtype, reverse=True)
            assert fwd.tobytes() == bwd.tobytes()
            assert fwd.tobytes() == np.asarray(M @ vec, dtype=dtype).tobytes()


@pytest.mark.parametrize("sizes", [(1, 256, 257), (257, 256, 255, 1)], ids=SC.size_id)
def test_recurrence_on_the_real_variant_is_well_conditioned(sizes):
    """The m = 10 recurrence the GPU test compares at 1e-11 must itself be
    determined to that level: under a 1e-16 relative perturbation of every
    HVP the oracle's alphas and betas move by less than 1e-13, and no beta
    comes near the 1e-6 breakdown threshold."""
    A = SC.crafted_case(sizes, "rows", seed=12)
    x = np.full(A.shape[1], 0.5)
    g = O.gradient(A, O.labels01(SC.labels(A.shape[0], 5)), x)
    w = O.hessian_weights(A, x)
    _, al, be, _ = O.lanczos(lambda z: O.hvp_from_weights(A, w, z), g, 10)
    assert len(al) == 10 and be.min() > 1e-5
    for trial in range(3):
        rng = np.random.default_rng(trial)

        def op(z):
            y = O.hvp_from_weights(A, w, z)
            return y * (1 + 1e-16 * rng.standard_normal(len(y)))

        _, al2, be2, _ = O.lanczos(op, g, 10)
        assert rel_err(al2, al) < 1e-13 and rel_err(be2, be) < 1e-13


# the nonzeros of every rank's block under a column cut of the breakdown fixtures
EMPTY_BLOCKS = {
    ("r1_", 2): [64, 0],
    ("r1_", 3): [64, 0, 0],
    ("r1_", 8): [64, 0, 0, 0, 0, 0, 0, 0],
    ("r3_", 2): [128, 64],
    ("r3_", 3): [64, 64, 64],
    ("r3_", 8): [64, 0, 64, 0, 0, 64, 0, 0],
}


@pytest.mark.parametrize("prefix,world", sorted(EMPTY_BLOCKS))
def test_breakdown_fixtures_cut_by_columns_leave_ranks_without_nonzeros(f2, prefix, world):
    A = golden_csr(f2, prefix)
    bounds, nnz = SC.block_nnz(A, world, "cols")
    assert nnz == EMPTY_BLOCKS[(prefix, world)]
    assert np.all(np.diff(bounds) >= 1)   # yet every rank has columns: it joins every collective


def test_rows_cut_with_every_nonzero_in_row_zero():
    A = sp.csr_matrix((np.arange(1.0, 6.0), np.array([0, 2, 3, 5, 6], dtype=np.int32),
                       np.array([0, 5, 5, 5, 5], dtype=np.int32)), shape=(4, 7))
    bounds, nnz = SC.block_nnz(A, 2, "rows")
    assert list(bounds) == [0, 1, 4]
    assert nnz == [5, 0]


def test_labels_and_integer_vectors():
    for n in (1, 2, 8, 514):
        b = SC.labels(n, 5)
        assert set(np.unique(b)) <= {-1.0, 1.0} and (n < 2 or len(np.unique(b)) == 2)
    w = SC.integer_vector(1000, 0, 4, 4)
    assert w.min() == 0 and w.max() == 4 and np.all(w == np.round(w))
    v = SC.integer_vector(1000, -3, 3, 1, nonzero=True, ends=2)
    assert set(np.unique(v)) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0} and v[0] == v[-1] == 2
