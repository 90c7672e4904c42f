"""krcn_cg_solve (csrc/krcn_cg.hpp, krcn_cg.hip) against the reference loop
oracle/krcn_oracle.py: cg, iterate by iterate and at the length edges.

krcn_cubic_cg's closing solve is compared with this call bitwise
(tests/test_gpu_cubic_cg.py), so whatever it gets wrong its caller reproduces.
The cases, their iteration counts and the conditions that make a comparison to
the iteration meaningful (margins of the stopping test, the reference's own
spread of 1e-13 under a reordering of its sums, three-iteration termination of
the diagonal construction) are built and asserted on the CPU in
tests/test_oracle_cg.py; this file imports them.

Bounds: 1e-12 on an iterate and its ||r_k|| (ten times the spread the CPU file
allows the reference alone); 1e-8 against the dense solve (the project's bound,
tests/test_gpu_methods.py); 1e-12 ||b|| between the reported and the true
residual; element-wise 1e-13 / 1e-6 on the diagonal cases (ten times what the
reference loop reaches); fp32 at four times the float32 reference's own error.

What each test would catch is in its docstring, argued from the code.
"""
import numpy as np
import pytest
import torch

import krcn
from conftest import rel_err
from test_gpu_reduce_edges import GUARD, inside
from test_oracle_cg import (CASES, DIAG_D, DIAG_RTOL, DIAG_SHIFT, DIAG_TOL, ITERATE_CASE, ITERATE_KS, ITERATIONS, RTOL,
                            case_id, dense_solution, diag_iterations, diag_problem, reference, reference_f32,
                            shifted_op, synth_problem)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
DT = {"fp64": (np.float64, F64, 1e300), "fp32": (np.float32, F32, 1e30)}
POLICIES = {"auto": {},
            "window-jag": dict(pass_formats=(krcn.KRCN_FORMAT_WINDOW, krcn.KRCN_FORMAT_JAG)),
            "sorted-sliced": dict(fmt=krcn.KRCN_FORMAT_SORTED, slicing=8)}
LONGEST = (12, 1e-5)     # 86 iterations: five flag checks pass before the one that sees `done`
MAXITER = 200            # above every count here (86 at most): a solver that fails to converge fails its test at once


def t(a, dtype=F64):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)      # (a copy: the shared inputs are read-only)


def h(x):
    return x.cpu().numpy()


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(seed, dtype=F64, policy="auto"):
        key = (seed, dtype, policy)
        if key not in made:
            made[key] = krcn.DeviceCSR(synth_problem(seed)[0], dtype=dtype, **POLICIES[policy])
        return made[key]

    yield get
    for X in made.values():
        X.close()


# ------------------------------------------------------------- the iterates
@pytest.mark.parametrize("K", ITERATE_KS)
def test_iterate_K_matches_the_reference(handles, K):
    """x_K and ||r_K|| of seed 8 at shift 1e-5 (44 iterations to 1e-10), stopped
    by maxiter = K at rtol 0, against the reference stopped at the same K.

    Would catch: k_cg_update reading rho[(k + 1) & 1] (at k = 0 that slot is 0,
    so alpha = 0 and x_1 = 0; later the ratio of successive rho, an order-one
    factor on every step); k_cg_dir writing iters = k (iterations == K fails,
    and residual_norm is then read from the other slot, the previous ||r||);
    beta formed from the wrong slot (beta = 1: x_2 is off by order one while
    the solve still converges, in more iterations, to 1e-8); a host loop whose
    flag check at k = 16 or 32 consumes the iteration (K = 17 and 33 report 16
    and 32 updates, K = 16 and 32 are unaffected).  K covers both parities of
    the rho double buffer on both sides of each check.

    Measured on an MI355X: x_K within 4.8e-16 and ||r_K|| within 7.0e-16 of the
    reference over the nine K."""
    seed, shift = ITERATE_CASE
    _, w, b = synth_problem(seed)
    x_ref, its, conv, rn = reference(seed, shift, K)
    assert its == K and not conv
    x, info = handles(seed).cg_solve(t(w), t(b), shift=shift, rtol=0.0, maxiter=K)
    ex = rel_err(h(x), x_ref)
    er = abs(info.residual_norm - rn[K]) / rn[K]
    print(f"K = {K}: x_K rel {ex:.2e}, ||r_K|| rel {er:.2e}")
    assert (info.converged, info.iterations, info.info) == (0, K, K)
    assert er <= 1e-12
    assert ex <= 1e-12


# -------------------------------------- counts past the first flag check
@pytest.mark.parametrize("case,policy", [(c, "auto") for c in CASES] + [(LONGEST, "window-jag"), (LONGEST, "sorted-sliced")],
                         ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_counts_solutions_and_reported_residual(handles, case, policy):
    """The six cases at rtol 1e-10: 7 / 24 / 44 and 6 / 23 / 86 iterations, the
    counts the reference takes (their margins: test_oracle_cg.py).  The
    86-iteration case also on window-slices + jagged plans and on sliced sorted
    plans, where the combine kernels run EpiCgQ.

    Would catch: an iteration count taken from the host's loop index (the host
    sees `done` only at the next multiple of 16: 86 would read 96); a stopping
    test on rho instead of sqrt(rho), or against rtol instead of rtol ||b||
    (the counts move by many iterations); residual_norm read from
    rho[(iters + 1) & 1] (the ||r|| before the last, at least 1.09 atol here,
    against a true residual below 0.9 atol: both parities occur); an epilogue
    whose p.q partials miss a slice (alpha is wrong: x fails 1e-8 or the count
    moves).

    Measured on an MI355X: counts equal on every case and policy; x within
    9.5e-11 of the dense solve (5.7e-12 at the 7-iteration case); reported
    against true residual within 2.7e-16 ||b|| (seed 12 at shift 1e-5, the 86
    iterations; below 1e-17 ||b|| on the other five)."""
    seed, shift = case
    A, w, b = synth_problem(seed)
    x, info = handles(seed, policy=policy).cg_solve(t(w), t(b), shift=shift, rtol=RTOL, maxiter=MAXITER)
    xs = h(x)
    nb = np.linalg.norm(b)
    true = np.linalg.norm(b - shifted_op(A, w, shift)(xs))
    ex = rel_err(xs, dense_solution(seed, shift))
    print(f"{case_id(case)} {policy}: {info.iterations} iterations, x rel {ex:.2e}, "
          f"| reported - true ||r|| | = {abs(info.residual_norm - true) / nb:.2e} ||b||")
    assert info.iterations == reference(seed, shift)[1] == ITERATIONS[case]
    assert (info.converged, info.info) == (1, 0)
    assert ex <= 1e-8
    assert abs(info.residual_norm - true) <= 1e-12 * nb
    assert info.residual_norm < RTOL * nb


# ------------------------------------------- every element, at the length edges
@pytest.mark.parametrize("d", DIAG_D)
@pytest.mark.parametrize("prec", list(DT))
def test_every_element_once_at_length_edges(prec, d):
    """The diagonal construction of test_oracle_cg.py: H + 0.5 I is diagonal with
    the values 0.75, 1.0 and 0.5 cycling with the column, all three in the last
    three columns, so CG ends in three iterations (one at d = 1) at
    x_c = b_c / H_cc, b small integers with b[-1] != 0.  d runs over a wave, a
    block, the 1024-block cap of vec_grid and the second to fourth trips of the
    grid-stride loops.  b sits between neighbours that would swamp rho, w
    between NaNs, and `out` between canaries.

    Would catch: an element dropped or visited twice by k_cg_begin (x, r or p
    keeps what the buffer held, or rho_0 misses b_c^2), by k_cg_update (x_c
    misses an alpha p_c or takes it twice: an order-one error in that element;
    r.r is off, which moves the count), by k_cg_dir (p_c is stale from the
    second iteration on) or by EpiCgQ (q_c stale, p.q off); a loop bound of
    d - 1 (b[-1] != 0 and the last column's value make x[-1] wrong) or d + 1
    (the neighbour of b enters rho_0: atol becomes huge and the solve stops
    after one iteration; the canary after `out` is overwritten).

    Measured on an MI355X: the largest element-wise relative error over all d
    is 2.2e-16 in fp64 and 1.19e-7 in fp32 (one ulp each); 3 iterations at
    every d >= 63, 1 at d = 1."""
    npdt, tdt, big = DT[prec]
    A, w, b, hd = diag_problem(d)
    X = krcn.DeviceCSR(A, dtype=tdt)
    _, bv = inside(b.astype(npdt), tdt, big)
    _, wv = inside(w.astype(npdt), tdt, float("nan"))
    canary = -7.0
    buf, out = inside(np.full(d, canary, dtype=npdt), tdt, canary)
    x, info = X.cg_solve(wv, bv, shift=DIAG_SHIFT, rtol=DIAG_RTOL[prec], maxiter=10, out=out)
    assert x.data_ptr() == out.data_ptr()
    xs = h(x).astype(np.float64)
    ref = b / hd
    nz = b != 0
    err = (np.abs(xs - ref)[nz] / np.abs(ref)[nz]).max()
    print(f"{prec} d = {d}: {info.iterations} iterations, element-wise rel {err:.2e}")
    assert (buf[:GUARD] == canary).all() and (buf[GUARD + d:] == canary).all(), "wrote outside the output"
    assert (info.converged, info.info, info.iterations) == (1, 0, diag_iterations(d))
    assert not xs[~nz].any()
    assert err <= DIAG_TOL[prec]
    X.close()


# ------------------------------------------- fp32 against its own reference
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fp32_against_the_float32_reference(handles, case):
    """An fp32 handle at rtol = 10 eps32 (what Cubic_LS passes) against the
    reference loop run in float32 (float32 vectors, alpha and beta; float64
    sums, as the device) on the float32-rounded inputs.  Both run one loop and
    differ in the order of their sums, so the device's error against the fp64
    dense solve of those inputs is held to four times the reference's, and its
    count to +-2 of the reference's.

    Would catch: sums accumulated in fp32 (the partials are double by
    contract), alpha or beta rounded twice, an fp32 path of the epilogue that
    forms s / n + shift p differently from the HVP's; the 1e-3 that
    test_gpu_placement.py allows an fp32 solve is three orders looser.

    Measured on an MI355X (device error / float32 reference's error,
    iterations device / reference):
      seed 8   shift 0.05  3.76e-07 / 3.76e-07   4 / 4
               shift 1e-3  4.51e-07 / 4.21e-07  15 / 15
               shift 1e-5  7.69e-07 / 8.87e-07  27 / 27
      seed 12  shift 0.05  1.25e-07 / 1.25e-07   4 / 4
               shift 1e-3  7.33e-07 / 7.41e-07  14 / 14
               shift 1e-5  1.81e-06 / 1.81e-06  52 / 52"""
    seed, shift = case
    _, w, b = synth_problem(seed)
    x_ref, its_ref, conv_ref, _ = reference_f32(seed, shift)
    dense = dense_solution(seed, shift, True)
    yard = rel_err(x_ref, dense)
    x, info = handles(seed, dtype=F32).cg_solve(t(w, F32), t(b, F32), shift=shift,
                                                rtol=10 * float(np.finfo(np.float32).eps), maxiter=MAXITER)
    err = rel_err(h(x), dense)
    print(f"{case_id(case)}: device {err:.2e} in {info.iterations} iterations, float32 reference {yard:.2e} in {its_ref}")
    assert conv_ref and info.converged == 1 and info.info == 0
    assert abs(info.iterations - its_ref) <= 2
    assert err <= 4 * yard


# ------------------------------------------------------- state between calls
def test_no_state_survives_a_call(handles):
    """A converged solve, a solve stopped at maxiter = 3, b = 0 (which sets
    `done` without an iteration) and the first solve again, on one handle: the
    fourth result is the first bitwise, and a fresh handle's.  maxiter = 0
    leaves x = 0 and, by the header (info: 0 converged, maxiter if not),
    info == maxiter == 0 with converged == 0 telling the two apart.

    Would catch: k_cg_init keeping `done`, `iters` or rho[1] of the previous
    call (the solve after b = 0 would return at once with x = 0; after the
    stopped solve iterations would start from 3); k_cg_begin not clearing x;
    the workspace r | p | q reused without r = p = b."""
    seed, shift = 8, 1e-3
    A, w, b = synth_problem(seed)
    X = handles(seed)
    wd, bd = t(w), t(b)

    def fields(i):
        return (i.converged, i.info, i.iterations, i.residual_norm)

    x1, i1 = X.cg_solve(wd, bd, shift=shift, rtol=RTOL, maxiter=MAXITER)
    assert fields(i1)[:3] == (1, 0, ITERATIONS[(seed, shift)])
    x1 = x1.clone()
    x2, i2 = X.cg_solve(wd, bd, shift=shift, rtol=RTOL, maxiter=3)
    assert fields(i2)[:3] == (0, 3, 3)
    assert rel_err(h(x2), reference(seed, shift, 3)[0]) <= 1e-12
    x3, i3 = X.cg_solve(wd, torch.zeros_like(bd), shift=shift, rtol=RTOL, maxiter=MAXITER)
    assert fields(i3) == (1, 0, 0, 0.0) and not x3.any()
    x4, i4 = X.cg_solve(wd, bd, shift=shift, rtol=RTOL, maxiter=MAXITER)
    assert torch.equal(x4, x1) and fields(i4) == fields(i1)
    Y = krcn.DeviceCSR(A)
    x5, i5 = Y.cg_solve(wd, bd, shift=shift, rtol=RTOL, maxiter=MAXITER)
    assert torch.equal(x5, x1) and fields(i5) == fields(i1)
    Y.close()
    out = torch.full_like(bd, 9.0)
    x0, i0 = X.cg_solve(wd, bd, shift=shift, rtol=RTOL, maxiter=0, out=out)
    assert not x0.any()
    assert fields(i0) == (0, 0, 0, float(np.linalg.norm(b)))


# ------------------------------------------------ non-finite never converges
def test_non_finite_never_reports_convergence():
    """A right-hand side with one NaN, and shift = 0 with b supported on an empty
    column (H p = 0, so p.q = 0 and alpha = rho / 0): every comparison with a
    NaN is false, so the solve runs its maxiter = 20 updates, returns KRCN_OK
    and reports converged == 0 with iterations == 20.

    Would catch: a stopping test written as !(sqrt(rho) >= atol), which a NaN
    passes; `done` set by rho == 0 being evaluated on a NaN-contaminated sum
    with a comparison that holds for NaN; a host loop that waits for `done`
    instead of counting to maxiter."""
    d = 65
    A, w, b, _ = diag_problem(d)
    X = krcn.DeviceCSR(A)
    wd = t(w)
    bn = b.copy()
    bn[7] = np.nan
    x, info = X.cg_solve(wd, t(bn), shift=DIAG_SHIFT, rtol=1e-10, maxiter=20)
    assert (info.converged, info.info, info.iterations) == (0, 20, 20)
    assert np.isnan(info.residual_norm)
    e = np.zeros(d)
    e[2] = 1.0                                   # column 2 is empty: H e = 0
    assert not shifted_op(A, w, 0.0)(e).any()
    x, info = X.cg_solve(wd, t(e), shift=0.0, rtol=1e-10, maxiter=20)
    assert (info.converged, info.info, info.iterations) == (0, 20, 20)
    assert not np.isfinite(h(x)).all()
    X.close()
