"""krcn_cubic_cg on the GPU: the full-space cubic subproblem, Newton over CG in
one call (DeviceCSR.cubic_cg, Cubic_LS(device_solver=True)).

Problems: synth seed 8 (2000 x 700, nnz 40 000) and seed 12 (1500 x 900, nnz
20 000) at x = 0.5 * 1 — d is no multiple of 256, so the vector kernels span
several blocks with a ragged last one —, w = O.hessian_weights, g = O.gradient
with the l2 term.

Bounds.  Against the dense host solver (optimizer.cubic.cubic_solver_root on H
formed in numpy) at cg_rtol 1e-10: equal solver_it; lam and model_decrease
within 1e-12 relative; s within 1e-8 relative (test_cg_solve_matches_dense_solve's
bound at this rtol).  Measured on an MI355X: lam <= 1.2e-16,
model_decrease <= 2.4e-16, s <= 2.6e-11.  Against the existing CG: bitwise.
"""
import functools

import numpy as np
import pytest
import torch

import krcn
import krcn_oracle as O
from conftest import load_golden, rel_err
from krcn import synth
from optimizer.cubic import Cubic_LS, cubic_solver_root
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = {8: (2000, 700, 40_000), 12: (1500, 900, 20_000)}
# (seed, l2, M), all with cg_rtol 1e-10
CASES = [(8, 0.0, 1.0), (8, 0.01, 5e-4), (12, 0.01, 1.0)]
RTOL = 1e-10


@functools.lru_cache(maxsize=None)
def problem(seed):
    n, d, nnz = SHAPES[seed]
    A, b = synth.make_problem(None, seed=seed, n=n, d=d, nnz=nnz)
    x = np.full(d, 0.5)
    w = O.hessian_weights(A, x)
    return A, O.labels01(b), x, w, krcn.DeviceCSR(A), torch.from_numpy(w).to(DEV)


def gradient(seed, l2):
    A, b01, x, _, _, _ = problem(seed)
    return O.gradient(A, b01, x, l2)


@functools.lru_cache(maxsize=None)
def host_solution(seed, l2, M):
    """The dense host solver on H formed in numpy; computed once per case."""
    A, _, _, w, _, _ = problem(seed)
    H = (A.T.multiply(w) @ A / A.shape[0]).toarray() + l2 * np.eye(A.shape[1])
    return cubic_solver_root(gradient(seed, l2), H, M, 100, 1e-8, 0.1)


def device_solution(seed, l2, M, **kw):
    X, wd = problem(seed)[4:]
    g = torch.from_numpy(gradient(seed, l2)).to(DEV)
    kw.setdefault("cg_rtol", RTOL)
    s, info = X.cubic_cg(wd, g, M, l2=l2, **kw)
    return s, info, g


def finite(info):
    return all(np.isfinite(v) for v in (info.lam, info.model_decrease, info.s_norm, info.reg_coef))


# ------------------------------------------------- 1. against the dense host solver
@pytest.mark.parametrize("seed,l2,M", CASES)
def test_matches_the_dense_host_solver(seed, l2, M):
    s_ref, its_ref, lam_ref, dec_ref = host_solution(seed, l2, M)
    s, info, _ = device_solution(seed, l2, M)
    e_lam = abs(info.lam - lam_ref) / abs(lam_ref)
    e_dec = abs(info.model_decrease - dec_ref) / abs(dec_ref)
    e_s = rel_err(s.cpu().numpy(), s_ref)
    print(f"seed {seed} l2 {l2} M {M}: its {info.solver_it} (host {its_ref}) lam {e_lam:.2e} dec {e_dec:.2e} "
          f"s {e_s:.2e} solves {info.cg_solves} cg_iterations {info.cg_iterations} ticks {info.ticks}")
    assert info.solver_status == 0 and info.reg_coef == M
    assert info.solver_it == its_ref
    assert e_lam <= 1e-12 and e_dec <= 1e-12
    assert e_s <= 1e-8


# ------------------------------------------------- 2. pinned to the existing CG, bitwise
@pytest.mark.parametrize("seed,l2,M,it_max", [c + (100,) for c in CASES] + [c + (1,) for c in CASES])
def test_closing_solve_is_cg_solve_bitwise(seed, l2, M, it_max):
    X, wd = problem(seed)[4:]
    s, info, g = device_solution(seed, l2, M, it_max=it_max)
    assert info.solver_status == (3 if it_max == 1 else 0)
    assert info.solver_it <= it_max
    y, cg = X.cg_solve(wd, g, shift=l2 + info.lam, rtol=RTOL, maxiter=10 * X.d)
    assert cg.converged == 1
    assert torch.equal(s, -y)
    ns = X.diff_norm(s)
    assert info.s_norm == ns
    dec = info.lam / 2 * (ns * ns) - M / 3 * (ns * ns * ns) - X.dot(g, s) / 2
    assert abs(info.model_decrease - dec) <= 1e-14 * abs(dec)


# ------------------------------------------------- 3. counters
@pytest.mark.parametrize("seed,l2,M", CASES)
def test_counters(seed, l2, M):
    _, info, _ = device_solution(seed, l2, M)
    assert info.cg_solves == 2 * info.solver_it + 1
    assert info.cg_iterations > 0 and info.cg_unconverged == 0
    assert info.ticks >= info.cg_iterations          # every x-update is one tick; the last batch may overshoot


def test_solves_that_stop_at_cg_maxiter_are_counted():
    seed, l2, M = CASES[1]
    s, info, _ = device_solution(seed, l2, M, cg_maxiter=2)
    assert info.solver_status in (0, 3)
    assert info.cg_unconverged == info.cg_solves > 0
    assert info.cg_iterations == 2 * info.cg_solves
    assert finite(info) and bool(torch.isfinite(s).all())


# ------------------------------------------------- 4. g = 0
def test_zero_gradient_halves_lam():
    X, wd = problem(8)[4:]
    M, r0, eps = 1.0, 0.1, 1e-8
    s, info = X.cubic_cg(wd, torch.zeros(X.d, dtype=torch.float64, device=DEV), M, r0=r0, eps=eps, cg_rtol=RTOL)
    p0, its = r0, 0
    for itr in range(100):          # the state rule's three expressions with ||y|| = y.z = 0
        fval = p0 * p0 - M * M * (0.0 * 0.0)
        fder = 2.0 * p0 - M * M * (-2.0 * 0.0)
        p = p0 - fval / fder
        its = itr + 1
        if p == p0 or abs(p - p0) <= eps:
            break
        p0 = p
    assert info.solver_status == 0 and info.solver_it == its and info.lam == p
    assert info.cg_iterations == 0 and info.cg_solves == 2 * its + 1
    sh = s.cpu().numpy()
    assert not np.isnan(sh).any() and not sh.any()
    assert info.s_norm == 0.0 and info.model_decrease == 0.0


# ------------------------------------------------- 5. d = 1 and fp32
def test_a_single_column():
    rng = np.random.default_rng(5)
    import scipy.sparse as sp
    A = sp.csr_matrix(rng.standard_normal((64, 1)))
    w = np.full(64, 0.2)
    g = np.array([0.3])
    X = krcn.DeviceCSR(A)
    s, info = X.cubic_cg(torch.from_numpy(w).to(DEV), torch.from_numpy(g).to(DEV), 1.0, l2=0.01, cg_rtol=RTOL)
    H = (A.T.multiply(w) @ A / 64).toarray() + 0.01 * np.eye(1)
    s_ref, its_ref, lam_ref, dec_ref = cubic_solver_root(g, H, 1.0, 100, 1e-8, 0.1)
    assert info.solver_status == 0 and info.solver_it == its_ref and info.cg_unconverged == 0
    assert abs(info.lam - lam_ref) <= 1e-12 * lam_ref and abs(info.model_decrease - dec_ref) <= 1e-12 * abs(dec_ref)
    assert rel_err(s.cpu().numpy(), s_ref) <= 1e-8


def test_an_fp32_handle():
    seed, l2, M = CASES[1]
    A = problem(seed)[0]
    s64, info64, _ = device_solution(seed, l2, M)
    X32 = krcn.DeviceCSR(A, dtype=torch.float32)
    w32 = problem(seed)[5].to(torch.float32)
    g32 = torch.from_numpy(gradient(seed, l2)).to(DEV, torch.float32)
    s32, info32 = X32.cubic_cg(w32, g32, M, l2=l2, cg_rtol=10 * float(torch.finfo(torch.float32).eps))
    assert s32.dtype == torch.float32 and info32.solver_status in (0, 3)
    assert info32.cg_unconverged == 0
    assert rel_err(s32.cpu().numpy(), s64.cpu().numpy()) <= 1e-4


# ------------------------------------------------- 6. workspace and scratch
def test_second_call_allocates_nothing_and_scratch_is_shared_safely():
    seed, l2, M = CASES[1]
    A, _, _, _, _, wd = problem(seed)
    g = torch.from_numpy(gradient(seed, l2)).to(DEV)

    def probes(X):
        y, ci = X.cg_solve(wd, g, shift=0.05, rtol=1e-10)
        V, al, be, li = X.lanczos(wd, g, 10, l2=l2)
        return y.clone(), ci.iterations, V.clone(), al, be, li.m_eff

    fresh = probes(krcn.DeviceCSR(A))
    X = krcn.DeviceCSR(A)
    before = probes(X)
    s1, info1 = X.cubic_cg(wd, g, M, l2=l2, cg_rtol=RTOL)
    bytes1 = X.owned_bytes()
    s2, info2 = X.cubic_cg(wd, g, M, l2=l2, cg_rtol=RTOL)
    assert X.owned_bytes() == bytes1
    assert torch.equal(s1, s2) and info1.lam == info2.lam and info1.cg_iterations == info2.cg_iterations
    after = probes(X)
    for got in (before, after):
        assert torch.equal(got[0], fresh[0]) and got[1] == fresh[1]
        assert torch.equal(got[2], fresh[2])
        np.testing.assert_array_equal(got[3], fresh[3])
        np.testing.assert_array_equal(got[4], fresh[4])
        assert got[5] == fresh[5]
    # the call's own buffers: one d-vector and the 16,512-byte state block on top of cg_solve's
    Xc = krcn.DeviceCSR(A)
    Xc.cg_solve(wd, g, shift=0.05, rtol=1e-10)
    b0 = Xc.owned_bytes()
    Xc.cubic_cg(wd, g, M, l2=l2, cg_rtol=RTOL)
    assert Xc.owned_bytes() - b0 == 8 * Xc.d + 16512


# ------------------------------------------------- 7. the optimizer
def test_cubic_ls_with_the_device_solver():
    f6 = load_golden("f6_methods.npz")
    n, d, nnz = (int(v) for v in f6["shape"])
    A, b = synth.make_problem(None, seed=int(f6["seed"]), n=n, d=d, nnz=nnz)
    runs = {}
    for dev in (False, True):
        loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
        opt = Cubic_LS(loss=loss, reg_coef=1e-3, label="CRN", cubic_solver="CG", tolerance=1e-8, tqdm=False,
                       device_solver=dev)
        tr = opt.run(x0=np.full(A.shape[1], 0.5), it_max=3)
        opt.compute_loss_of_iterates()
        runs[dev] = (opt, tr)
    opt, tr = runs[True]
    assert opt.cg_iterations > 0 and opt.cg_unconverged == 0
    np.testing.assert_allclose(tr.loss_vals, f6["full_loss_vals"], rtol=1e-6)
    assert rel_err(np.asarray(tr.xs), f6["full_xs"]) < 1e-5
    host, tr_host = runs[False]
    assert opt.reg_coef == host.reg_coef
    its, its_host = np.diff(tr.solver_its), np.diff(tr_host.solver_its)
    assert len(its) == len(its_host) == 3 and np.abs(its - its_host).max() <= 1


# ------------------------------------------------- failures end the chain with s zeroed
def test_a_nan_in_g_is_status_4():
    X, wd = problem(8)[4:]
    g = torch.from_numpy(gradient(8, 0.0)).to(DEV).clone()
    g[300] = float("nan")
    out = torch.full((X.d,), 7.0, dtype=torch.float64, device=DEV)
    s, info = X.cubic_cg(wd, g, 1.0, cg_rtol=RTOL, out=out)
    assert info.solver_status == 4 and info.cg_iterations == 0 and info.cg_solves == 0 and info.ticks >= 1
    assert not s.cpu().numpy().any()


def test_an_indefinite_operator_is_status_1():
    X, wd = problem(8)[4:]
    g = torch.from_numpy(gradient(8, 0.0)).to(DEV)
    # l2 = -1000 puts every eigenvalue of H + (l2 + r0) I far below zero: p.q < 0 in the first iteration
    s, info = X.cubic_cg(wd, g, 1.0, l2=-1000.0, cg_rtol=RTOL)
    assert info.solver_status == 1 and info.solver_it == 0 and info.cg_solves == 1
    assert not s.cpu().numpy().any()
