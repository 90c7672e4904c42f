"""The Krylov-CRN step behind one library call (krcn_crn_step) and its device
subproblem (krcn_cubic_tridiag) against the host path they replace.

Tolerances: the subproblem at the host solver's own test tolerance (1e-13
relative, equal Newton iteration counts: tests/test_host_logic.py); fp64
trajectories at the host path's 1e-10 with equal line-search decisions
(tests/test_gpu_crn.py); fp32 at the project's fp32 CRN tolerance (1e-3 on x,
1e-4 on values: tests/test_gpu_configs.py).
"""
import numpy as np
import numpy.linalg as la
import pytest
import torch

import krcn
from conftest import rel_err
from krcn import _lib, synth
from optimizer import cubic as C
from optimizer.cubic import Cubic_Krylov_LS
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu

FIRST_BATCH = 2   # trials 0 and 1 go out before the host first reads the chain's state
BATCH = 4         # trials per later submission


@pytest.fixture(scope="module")
def f4_problem(f4):
    n, d, nnz = (int(v) for v in f4["shape"])
    return synth.make_problem(None, seed=int(f4["seed"]), n=n, d=d, nnz=nnz)


@pytest.fixture(scope="module")
def handle(f4_problem):
    X = krcn.DeviceCSR(f4_problem[0])
    yield X
    X.close()


def make_opt(A, b, device_step, reg_coef=1e-3, l2=0, dtype=torch.float64, m=10, **loss_kw):
    loss = LogisticRegression(A, b, l1=0, l2=l2, store_mat_vec_prod=True, dtype=dtype, **loss_kw)
    return Cubic_Krylov_LS(loss=loss, reg_coef=reg_coef, label="k", subspace_dim=m, tolerance=1e-9, tqdm=False,
                           device_step=device_step)


def host_trials(opt, reg0):
    """Backtracking trials of the host path's last step from its reg_coef:
    reg0 * beta / beta ** trials, every factor a power of two."""
    t = np.log2(opt.reg_coef / (reg0 * opt.beta))
    assert t == round(t)
    return int(round(t))


# ------------------------------------------------------------ the subproblem
def check_subproblem(X, g0, al, be, M, r0, ref):
    s, info = X.cubic_tridiag(al, be, g0, M, r0=r0, eps=1e-8)
    s_ref, its, lam, dec = ref
    assert info.solver_status == 0
    assert info.solver_it == its
    assert np.abs(s - s_ref).max() <= 1e-13 * np.abs(s_ref).max()
    assert abs(info.lam - lam) <= 1e-13 * abs(lam)
    assert abs(info.model_decrease - dec) <= 1e-13 * abs(dec)
    assert info.reg_coef == M


def test_subproblem_matches_golden(handle, f3):
    for m in (3, 10, 50):
        for k in range(3):
            key = f"m{m}_k{k}"
            T, g = f3[f"{key}_T"], f3[f"{key}_g"]
            assert np.count_nonzero(g[1:]) == 0
            check_subproblem(handle, g[0], np.diag(T), np.diag(T, 1), float(f3[f"{key}_M"]), float(f3[f"{key}_r0"]),
                             (f3[f"{key}_s"], int(f3[f"{key}_its"]), float(f3[f"{key}_r"]), float(f3[f"{key}_dec"])))


@pytest.mark.parametrize("m", [1, 2])
def test_subproblem_smallest_sizes(handle, m):
    al = np.array([0.7, 0.4])[:m]
    be = np.array([0.05])[:m - 1]
    g = np.zeros(m)
    g[0] = 0.3
    for M in (1e-3, 2.0):
        ref = C.cubic_solver_root_tridiag(g, al, be, M, epsilon=1e-8, r0=0.1)
        check_subproblem(handle, g[0], al, be, M, 0.1, ref)


def test_subproblem_it_max_returns_the_last_iterate(handle, f3):
    """root_scalar(method="newton") returns the last iterate without raising
    when maxiter runs out: status 3, the same root."""
    T, g = f3["m10_k0_T"], f3["m10_k0_g"]
    al, be, M = np.diag(T), np.diag(T, 1), float(f3["m10_k0_M"])
    s, info = handle.cubic_tridiag(al, be, g[0], M, r0=0.1, eps=1e-8, it_max=2)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s_ref, its, lam, dec = C.cubic_solver_root_tridiag(g, al, be, M, it_max=2, epsilon=1e-8, r0=0.1)
    assert info.solver_status == 3 and info.solver_it == its == 2
    assert abs(info.lam - lam) <= 1e-13 * abs(lam)
    assert np.abs(s - s_ref).max() <= 1e-13 * np.abs(s_ref).max()


def test_indefinite_input_is_a_status(handle):
    al, be = np.array([-5.0, 1.0, 1.0]), np.array([0.1, 0.1])
    with pytest.raises(la.LinAlgError):
        C.cubic_solver_root_tridiag(np.array([1.0, 0.0, 0.0]), al, be, 1e-3, r0=0.1)
    s, info = handle.cubic_tridiag(al, be, 1.0, 1e-3, r0=0.1)
    assert info.solver_status == 1
    assert not s.any()


def test_indefinite_shift_raises_through_the_optimizer(f4_problem):
    """A start r0 far below -lambda_min(T) leaves T + r0 I indefinite at the first
    Newton iterate: the host path raises LinAlgError from dpttrf, the device
    step reports status 1 and the optimizer raises the same error."""
    A, b = f4_problem
    for device_step in (False, True):
        opt = make_opt(A, b, device_step)
        opt.init_run(np.full(A.shape[1], 0.5))
        opt.r0 = -10.0
        x0 = opt.x.clone()
        with pytest.raises(la.LinAlgError, match="not positive definite"):
            opt.step()
        assert torch.equal(opt.x, x0)


# ------------------------------------------------------------------ the step
def test_trajectory_10_steps_device_step(f4, f4_problem):
    A, b = f4_problem
    d = A.shape[1]
    opt = make_opt(A, b, True)
    tr = opt.run(x0=np.full(d, 0.5), it_max=10)
    loss = opt.loss
    # the cache holds X x for the iterate the last step kept
    assert loss._cached(opt.x)
    assert loss.value(opt.x) == opt.value
    opt.compute_loss_of_iterates()
    xs = np.asarray(tr.xs)
    assert xs.shape == f4["xs"].shape
    assert rel_err(xs, f4["xs"]) < 1e-10
    assert tr.its == list(f4["its"])
    assert tr.solver_its == list(f4["solver_its"])
    np.testing.assert_allclose(tr.loss_vals, f4["loss_vals"], rtol=1e-10)
    assert opt.reg_coef == f4["final_reg_coef"]
    assert abs(opt.value - f4["final_value"]) <= 1e-10 * abs(f4["final_value"])


@pytest.fixture(scope="module")
def backtracking(f4_problem):
    """The host path's first step from a reg_coef so small that the line search
    rejects trials beyond the second submission of the device step."""
    A, b = f4_problem
    reg0 = 1e-9
    opt = make_opt(A, b, False, reg_coef=reg0)
    opt.run(x0=np.full(A.shape[1], 0.5), it_max=1)
    return reg0, opt


def test_backtracking_across_batch_boundaries(f4_problem, backtracking):
    A, b = f4_problem
    reg0, host = backtracking
    trials = host_trials(host, reg0)
    # trial indices 0..trials: past the first submission and past the second
    assert trials + 1 > FIRST_BATCH + BATCH
    assert trials < 20
    dev = make_opt(A, b, True, reg_coef=reg0)
    dev.run(x0=np.full(A.shape[1], 0.5), it_max=1)
    assert dev.reg_coef == host.reg_coef
    assert dev.solver_it == host.solver_it
    assert rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy()) < 1e-10
    assert abs(dev.value - host.value) <= 1e-10 * abs(host.value)


def test_trial_cap_keeps_the_last_trial(f4_problem, backtracking):
    A, b = f4_problem
    reg0, host = backtracking
    assert host_trials(host, reg0) > 2
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    X = loss.device_matrix
    x = loss.to_device(np.full(A.shape[1], 0.5))
    value = loss.value(x)
    Ax = loss._device_Ax(x)
    x_new, Ax_new, al, be, info = X.crn_step(x, loss._b_dev, value, 10, reg0, Ax=Ax, max_trials=2)
    assert info.accepted == 0 and info.trials == 2
    M = reg0 * 0.5 / 0.5 / 0.5
    assert info.reg_coef == M
    # the second backtracking trial by the host pieces
    V, al_h, be_h, li = X.lanczos(X.weights(Ax), loss.gradient(x), 10)
    np.testing.assert_array_equal(al, al_h)
    np.testing.assert_array_equal(be, be_h)
    g = np.zeros(len(al_h))
    g[0] = li.gnorm
    s, its, lam, dec = C.cubic_solver_root_tridiag(g, al_h, be_h, M, epsilon=1e-8, r0=0.1)
    want = X.basis_combine(V, s, x)
    assert rel_err(x_new.cpu().numpy(), want.cpu().numpy()) < 1e-10
    assert rel_err(Ax_new.cpu().numpy(), X.matvec(want).cpu().numpy()) < 1e-10
    assert info.solver_it == its
    assert abs(info.value_new - loss.value(want)) <= 1e-10 * abs(info.value_new)
    assert info.value_new > value - info.model_decrease
    assert info.dx_norm == X.diff_norm(x_new, x)


def two_paths(A, b, steps, **kw):
    out = []
    for device_step in (False, True):
        opt = make_opt(A, b, device_step, **kw)
        opt.run(x0=np.full(A.shape[1], 0.5), it_max=steps)
        out.append(opt)
    return out


def assert_same_decisions(host, dev):
    assert dev.it == host.it
    assert dev.reg_coef == host.reg_coef
    assert dev.solver_it == host.solver_it
    assert dev.last_lanczos.m_eff == host.last_lanczos.m_eff


def test_l2_three_steps(f4_problem):
    host, dev = two_paths(*f4_problem, 3, l2=0.01)
    assert_same_decisions(host, dev)
    assert rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy()) < 1e-10
    assert abs(dev.value - host.value) <= 1e-10 * abs(host.value)
    assert dev.loss._cached(dev.x)
    assert dev.loss.value(dev.x) == dev.value


def test_fp32_two_steps(f4_problem):
    """fp32 handle: the subproblem is fp64 on both paths and s is rounded to
    fp32 by the same expression in x + V^T s, so the two paths differ only
    where the device solver's s differs from LAPACK's in its last fp64 bits.
    Measured on an MI355X: x and the value are bitwise equal after two steps
    (relative distance 0 on both).  The bounds are the margins the project's
    fp32 CRN test gives itself (tests/test_gpu_configs.py: 1e-3 on x, 1e-4 on
    values)."""
    host, dev = two_paths(*f4_problem, 2, dtype=torch.float32)
    assert_same_decisions(host, dev)
    ex = rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy())
    ev = abs(dev.value - host.value) / abs(host.value)
    print(f"fp32 device step vs host path: x rel {ex:.3e}, value rel {ev:.3e}")
    assert ex < 1e-3
    assert ev < 1e-4


def test_dense_format_two_steps():
    A, b = synth.make_dense_problem(301, 301, 0.1, seed=8)
    host, dev = two_paths(A, b, 2, format="dense")
    assert dev.loss.device_matrix.plan_format() == {"pass1": "dense", "pass2": "dense"}
    assert_same_decisions(host, dev)
    assert rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy()) < 1e-10


def test_truncated_basis_one_step():
    """d < m: the recurrence breaks down and the device chain solves over the
    m_eff vectors the reference's truncation rule keeps."""
    A, b = synth.make_problem(None, seed=5, n=300, d=6, nnz=900)
    host, dev = two_paths(A, b, 1)
    assert host.last_lanczos.m_eff < 10
    assert_same_decisions(host, dev)
    assert rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy()) < 1e-10


def test_tolerance_stop_uses_the_reported_step_length(f4_problem):
    """With a tolerance that the first step's length already meets, both paths
    stop after that step."""
    A, b = f4_problem
    its = []
    for device_step in (False, True):
        opt = make_opt(A, b, device_step)
        opt.tolerance = 1e9
        opt.run(x0=np.full(A.shape[1], 0.5), it_max=5)
        its.append(opt.it)
        if device_step:
            assert opt.x_old_tol is None and opt._dx_norm > 0
    assert its == [1, 1]


def test_construction_refusals(f4_problem):
    A, b = f4_problem
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    with pytest.raises(ValueError):
        Cubic_Krylov_LS(loss=loss, reg_coef=1e-3, subspace_dim=10, tqdm=False, device_step=True,
                        dense_subproblem=True)


def test_sharded_handle_is_unsupported(f4_problem):
    A, b = f4_problem
    X = krcn.DeviceCSR(A, shard_mode=_lib.KRCN_SHARD_ROWS)
    x = torch.full((X.d,), 0.5, dtype=torch.float64, device=X.device)
    bd = torch.zeros(X.n, dtype=torch.float64, device=X.device)
    with pytest.raises(_lib.KrcnError) as e:
        X.crn_step(x, bd, 0.7, 10, 1e-3)
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    X.close()


def test_argument_ranges_are_invalid(handle):
    X = handle
    x = torch.full((X.d,), 0.5, dtype=torch.float64, device=X.device)
    bd = torch.zeros(X.n, dtype=torch.float64, device=X.device)
    for kw in ({"max_trials": -1}, {"ls_beta": 1.0}, {"ls_beta": 0.0}, {"solver_it_max": 0}):
        with pytest.raises(_lib.KrcnError) as e:
            X.crn_step(x, bd, 0.7, 10, 1e-3, **kw)
        assert e.value.status == _lib.KRCN_ERR_INVALID
    with pytest.raises(_lib.KrcnError) as e:
        X.crn_step(x, bd, 0.7, 2045, 1e-3, V=torch.empty((2045, X.d), dtype=torch.float64, device=X.device))
    assert e.value.status == _lib.KRCN_ERR_INVALID


def test_repeated_steps_allocate_nothing(f4_problem):
    A, b = f4_problem
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    X = loss.device_matrix
    x = loss.to_device(np.full(A.shape[1], 0.5))
    value = loss.value(x)
    V = torch.empty((10, X.d), dtype=torch.float64, device=X.device)
    sizes = []
    for _ in range(3):
        X.crn_step(x, loss._b_dev, value, 10, 1e-3, V=V)
        sizes.append(X.owned_bytes())
    assert sizes[1] == sizes[2]
    # a reserved handle's first step allocates nothing either
    Y = krcn.DeviceCSR(A)
    Y.reserve(10)
    before = Y.owned_bytes()
    Y.crn_step(x, loss._b_dev, value, 10, 1e-3, V=V)
    assert Y.owned_bytes() == before
    Y.close()
