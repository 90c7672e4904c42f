"""The reference conjugate gradients (oracle/krcn_oracle.py: cg) pinned on the
CPU, and the conditions under which tests/test_gpu_cg.py may compare the device
solver with it to the iteration, asserted on the reference alone.

The cases are built here and imported by the GPU file, so both see one set:
  synth cases   seed 8 (2000 x 700, nnz 40,000) and seed 12 (1500 x 900,
                nnz 20,000), w = hessian_weights at default_rng(1).uniform(-0.5,
                0.5), b = default_rng(2).standard_normal(d), shifts 0.05, 1e-3,
                1e-5, rtol 1e-10: 7/24/44 and 6/23/86 iterations;
  diagonal      X (d x d) with one unit nonzero per row, row i in column i
                except that rows with i % 3 == 2 go to column i - 1, and
                w = d t: H + 0.5 I is diagonal with the values 0.75 (columns
                c % 3 == 0), 1.0 (c % 3 == 1) and the bare shift 0.5 (the empty
                columns c % 3 == 2), so CG ends in three iterations (one at
                d = 1) at x_c = b_c / H_cc.

What is asserted:
  - x and the iteration count are scipy.sparse.linalg.cg's, bitwise;
  - the count is not at the mercy of a rounding: the final residual is below
    0.95 atol and the one before it above 1.05 atol;
  - the reference's own spread under a reordering of its sums (the dots over a
    fixed permutation of the unknowns, X^T u from a CSR of X^T instead of the
    CSC product) is at most 1e-13 relative on every ||r_k|| and x_k the GPU file
    compares (k <= 33), a tenth of its 1e-12;
  - the recursive residual is the true one to 1e-14 ||b||;
  - on the diagonal cases the reference takes three iterations and stays inside
    a tenth of the GPU file's element-wise bounds (1e-13 fp64, 1e-6 fp32), or
    inside one ulp where that tenth is less than one (float32: 1.19e-7).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import krcn_oracle as O
from conftest import rel_err
from krcn import synth

SHAPES = {8: dict(n=2000, d=700, nnz=40_000), 12: dict(n=1500, d=900, nnz=20_000)}
SHIFTS = (0.05, 1e-3, 1e-5)
CASES = [(seed, shift) for seed in SHAPES for shift in SHIFTS]
ITERATIONS = {(8, 0.05): 7, (8, 1e-3): 24, (8, 1e-5): 44, (12, 0.05): 6, (12, 1e-3): 23, (12, 1e-5): 86}
RTOL = 1e-10
ITERATE_CASE = (8, 1e-5)                          # test_gpu_cg.py compares its iterates one at a time
ITERATE_KS = (1, 2, 3, 15, 16, 17, 31, 32, 33)    # both parities, both sides of the host's flag check at 16 and 32

CAP = 256 * 1024
DIAG_D = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, CAP - 1, CAP, CAP + 1, CAP + 257, 3 * CAP + 1]
DIAG_SHIFT = 0.5
DIAG_RTOL = {"fp64": 1e-12, "fp32": 1e-5}
DIAG_TOL = {"fp64": 1e-13, "fp32": 1e-6}          # the GPU file's element-wise bounds
NPDT = {"fp64": np.float64, "fp32": np.float32}


def case_id(c):
    return f"seed{c[0]}-shift{c[1]:g}"


@functools.lru_cache(maxsize=None)
def synth_problem(seed):
    """(A, w, b) of a synth shape; read-only."""
    A, _ = synth.make_problem(None, seed=seed, **SHAPES[seed])
    d = A.shape[1]
    w = O.hessian_weights(A, np.random.default_rng(1).uniform(-0.5, 0.5, size=d))
    b = np.random.default_rng(2).standard_normal(d)
    for a in (w, b):
        a.setflags(write=False)
    return A, w, b


def shifted_op(A, w, shift, dtype=np.float64):
    """v -> X^T (w (.) X v) / n + shift v, the operator of krcn_cg_solve.  With
    dtype=np.float32 every array and every product is float32."""
    dt = np.dtype(dtype)
    A = sp.csr_matrix(A, dtype=dt)
    w = np.asarray(w, dtype=dt)
    n, s = dt.type(A.shape[0]), dt.type(shift)
    return lambda v: A.T @ (w * (A @ v)) / n + s * v


def dense_matrix(A, w, shift):
    A = sp.csr_matrix(A, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    return (A.T.multiply(w) @ A / A.shape[0]).toarray() + shift * np.eye(A.shape[1])


@functools.lru_cache(maxsize=None)
def dense_solution(seed, shift, f32_inputs=False):
    """np.linalg.solve on the dense H + shift I, of the inputs as given or rounded to float32."""
    A, w, b = synth_problem(seed)
    if f32_inputs:
        A, w, b = (sp.csr_matrix(A, dtype=np.float32), w.astype(np.float32), b.astype(np.float32))
    x = np.linalg.solve(dense_matrix(A, w, shift), np.asarray(b, dtype=np.float64))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(seed, shift, maxiter=None):
    """O.cg on a synth case at RTOL, or stopped after `maxiter` updates at rtol 0."""
    A, w, b = synth_problem(seed)
    out = O.cg(shifted_op(A, w, shift), b, RTOL if maxiter is None else 0.0, 10 * len(b) if maxiter is None else maxiter)
    out[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_f32(seed, shift):
    """O.cg in float32 on the float32-rounded inputs at rtol = 10 eps32 (what Cubic_LS passes)."""
    A, w, b = synth_problem(seed)
    out = O.cg(shifted_op(A, w, shift, np.float32), b.astype(np.float32), 10 * float(np.finfo(np.float32).eps),
               10 * len(b), dtype=np.float32)
    out[0].setflags(write=False)
    return out


def diag_problem(d):
    """(X, w, b, h): the diagonal construction of the module docstring; h is the
    diagonal of H + DIAG_SHIFT I.  w, b and h are exact in float32."""
    i = np.arange(d)
    cols = np.where(i % 3 == 2, i - 1, i)
    X = sp.csr_matrix((np.ones(d), cols.astype(np.int32), np.arange(d + 1, dtype=np.int32)), shape=(d, d))
    t = np.full(d, 0.25)
    if (d - 1) % 3 == 1:
        t[-1] = 0.5          # the last column has lost its second row: keep its value at 1.0
    b = np.random.default_rng(23).integers(-3, 4, d).astype(np.float64)
    b[-1] = 3.0
    h = np.bincount(cols, weights=t, minlength=d) + DIAG_SHIFT
    return X, d * t, b, h


def diag_iterations(d):
    return 3 if d >= 3 else 1


# ------------------------------------------------------------------- scipy
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cg_is_scipy_bitwise(case):
    A, w, b = synth_problem(case[0])
    op = shifted_op(A, w, case[1])
    seen = []
    x_sp, info = spla.cg(spla.LinearOperator((len(b), len(b)), matvec=op, dtype=np.float64), b, rtol=RTOL, atol=0.0,
                         callback=lambda xk: seen.append(1))
    x, its, conv, rn = reference(*case)
    assert info == 0 and conv
    assert its == len(seen) == ITERATIONS[case]
    assert np.array_equal(x, x_sp)
    assert len(rn) == its + 1 and rn[0] == np.linalg.norm(b)


def test_cg_stopped_at_maxiter_is_scipy_bitwise():
    A, w, b = synth_problem(ITERATE_CASE[0])
    lin = spla.LinearOperator((len(b), len(b)), matvec=shifted_op(A, w, ITERATE_CASE[1]), dtype=np.float64)
    full = reference(*ITERATE_CASE)[3]
    for K in ITERATE_KS:
        x_sp, info = spla.cg(lin, b, rtol=0.0, atol=0.0, maxiter=K)
        x, its, conv, rn = reference(*ITERATE_CASE, K)
        assert info == K and its == K and not conv
        assert np.array_equal(x, x_sp)
        assert rn == full[:K + 1]            # the stopped run is a prefix of the converged one
    x0, its0, conv0, rn0 = O.cg(lin.matvec, b, RTOL, 0)
    assert its0 == 0 and not conv0 and not x0.any() and rn0 == [np.linalg.norm(b)]
    xz, itsz, convz, rnz = O.cg(lin.matvec, np.zeros(len(b)), RTOL, 10)
    assert itsz == 0 and convz and not xz.any() and rnz == [0.0]
    assert spla.cg(lin, np.zeros(len(b)), rtol=RTOL, atol=0.0)[1] == 0


# ----------------------------------------------- conditions of the GPU tests
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_iteration_count_has_margin(case):
    _, w, b = synth_problem(case[0])
    _, its, _, rn = reference(*case)
    atol = RTOL * np.linalg.norm(b)
    print(f"{case_id(case)}: {its} iterations, last ||r|| = {rn[-1] / atol:.3f} atol, the one before {rn[-2] / atol:.3f} atol")
    assert rn[-1] < 0.95 * atol
    assert rn[-2] > 1.05 * atol


def reordered(seed, shift, maxiter=None):
    """The same solve with every sum in another order: the unknowns permuted (the
    dots run over the permuted vectors) and X^T u by the row loop over a CSR of
    X^T instead of the column scatter of the CSC product.  x comes back in
    the original order."""
    A, w, b = synth_problem(seed)
    perm = np.random.default_rng(7).permutation(len(b))
    inv = np.argsort(perm)
    At = sp.csr_matrix(A.T)
    At.sort_indices()
    n = A.shape[0]
    op = lambda v: (At @ (w * (A @ v[inv])) / n)[perm] + shift * v   # noqa: E731
    x, its, conv, rn = O.cg(op, b[perm], RTOL if maxiter is None else 0.0, 10 * len(b) if maxiter is None else maxiter)
    return x[inv], its, conv, rn


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_spread_under_reordering(case):
    x, its, _, rn = reference(*case)
    x2, its2, _, rn2 = reordered(*case)
    assert its2 == its
    # (CG amplifies a rounding from step to step: by k = 86 the two orders are 3e-3 apart on ||r_k||
    # with equal counts and solutions, which is why the iterates are compared up to k = 33 only)
    kmax = min(its, max(ITERATE_KS))
    spread = max(abs(a - c) / a for a, c in zip(rn[:kmax + 1], rn2[:kmax + 1]))
    late = max(abs(a - c) / a for a, c in zip(rn, rn2))
    print(f"{case_id(case)}: ||r_k|| spread {spread:.2e} over k = 0..{kmax} ({late:.2e} over k = 0..{its}), "
          f"x spread {rel_err(x2, x):.2e}")
    assert spread <= 1e-13
    assert rel_err(x2, x) <= 1e-9        # a tenth of the 1e-8 at which the solutions are compared
    if case == ITERATE_CASE:
        assert its >= max(ITERATE_KS)
        for K in ITERATE_KS:
            e = rel_err(reordered(*case, K)[0], reference(*case, K)[0])
            print(f"  x_{K} spread {e:.2e}")
            assert e <= 1e-13


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_recursive_residual_is_the_true_one(case):
    A, w, b = synth_problem(case[0])
    x, _, _, rn = reference(*case)
    true = np.linalg.norm(b - shifted_op(A, w, case[1])(x))
    gap = abs(true - rn[-1]) / np.linalg.norm(b)
    print(f"{case_id(case)}: | ||b - Hx|| - ||r|| | = {gap:.2e} ||b||")
    assert gap <= 1e-14


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_f32_reference_converges(case):
    """The yardstick of the GPU file's fp32 test exists and means something: the
    float32 loop converges, and its error against the dense solve is far inside
    the 1e-3 that tests/test_gpu_placement.py allows an fp32 solve."""
    x, its, conv, _ = reference_f32(*case)
    err = rel_err(x, dense_solution(*case, True))
    print(f"{case_id(case)}: float32 reference {its} iterations, error {err:.2e}")
    assert conv and x.dtype == np.float32
    assert 0 < err < 1e-5


@pytest.mark.parametrize("d", DIAG_D)
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_diagonal_cases_end_in_three_iterations(prec, d):
    X, w, b, h = diag_problem(d)
    dt = NPDT[prec]
    for a in (w, b, h):
        assert np.array_equal(a.astype(np.float32), a)
    want = {0.75, 1.0, 0.5} if d >= 3 else {0.75}
    assert set(np.unique(h)) == want and b[-1] != 0
    if d >= 3:
        assert np.array_equal(shifted_op(X, w, DIAG_SHIFT)(b), h * b)      # H + shift I is that diagonal
        assert set(np.unique(h[-3:])) == want                              # all three values at the very end
    x, its, conv, _ = O.cg(shifted_op(X, w, DIAG_SHIFT, dt), b.astype(dt), DIAG_RTOL[prec], 10 * d, dtype=dt)
    ref = b / h
    err = np.abs(x - ref)[b != 0] / np.abs(ref)[b != 0]
    assert conv and its == diag_iterations(d)
    assert not x[b == 0].any()
    # a tenth of the GPU bound; in float32 that tenth (1e-7) is below the format's own spacing
    # (eps32 = 1.19e-7 relative to an x_c in [1, 2)), which the loop reaches exactly: one ulp
    assert err.max() <= max(0.1 * DIAG_TOL[prec], np.finfo(dt).eps), f"d = {d}: {err.max():.2e}"
