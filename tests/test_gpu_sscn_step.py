"""The SSCN step behind one library call (krcn_sscn_step) and its device
subproblem (krcn_cubic_dense) against the reference's outputs and the host
path they replace.

Tolerances: the subproblem within max(1e-13, 2 eps cond) of the reference's
cubic_solver_root (1e-13 is the tridiagonal kernel's own test tolerance; cond is
stored with the ill-conditioned cases of tests/golden/f10_cubic_dense.npz),
equal Newton iteration counts at xtol = 1e-8 and within one at xtol = machine
epsilon, where the count sits on the last bit of lam.  fp64 trajectories at
the host test's 1e-10 with equal line-search decisions; fp32 at the project's
fp32 CRN margins (1e-3 on x, 1e-4 on values).
"""
import os
import re

import numpy as np
import pytest
import torch

import krcn
from conftest import PKG, golden_csr, load_golden, rel_err
from krcn import _lib, synth
from optimizer import cubic as C
from optimizer.cubic import SSCN
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu


def batch_sizes():
    """kCrnFirstBatch (trials 0 and 1 go out before the host first reads the chain's
    state) and kCrnBatch (trials per later submission), from the header both steps share."""
    text = open(os.path.join(PKG, "csrc", "krcn_cubic.hpp")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))
                 for name in ("kCrnFirstBatch", "kCrnBatch"))


FIRST_BATCH, BATCH = batch_sizes()
EPS = float(np.finfo(float).eps)


@pytest.fixture(scope="module")
def f6():
    return load_golden("f6_methods.npz")


@pytest.fixture(scope="module")
def f7():
    return load_golden("f7_coord.npz")


@pytest.fixture(scope="module")
def f10():
    return load_golden("f10_cubic_dense.npz")


@pytest.fixture(scope="module")
def f6_problem(f6):
    n, d, nnz = (int(v) for v in f6["shape"])
    A, b = synth.make_problem(None, seed=int(f6["seed"]), n=n, d=d, nnz=nnz)
    return A.tocsc(), b


@pytest.fixture(scope="module")
def handle(f7):
    X = krcn.DeviceCSR(golden_csr(f7))
    yield X
    X.close()


# ------------------------------------------------------------ the subproblem
def check_solve(X, H, g, M, eps, ref, bound, label):
    s, info = X.cubic_dense(H, g, M, r0=0.1, eps=eps)
    s_ref, its, lam, dec = ref
    es = la_norm(s - s_ref) / la_norm(s_ref)
    el = abs(info.lam - lam) / abs(lam)
    ed = abs(info.model_decrease - dec) / abs(dec)
    print(f"{label}: k {len(g)} M {M:g} eps {eps:g} its {info.solver_it}/{its} s {es:.2e} lam {el:.2e} "
          f"dec {ed:.2e} bound {bound:.2e}")
    assert info.solver_status == 0
    assert info.reg_coef == M
    assert es <= bound and el <= bound and ed <= bound
    if eps == 1e-8:
        assert info.solver_it == its
    else:
        assert abs(info.solver_it - its) <= 1


def la_norm(v):
    return float(np.linalg.norm(np.asarray(v, dtype=np.float64)))


def test_dense_subproblem_matches_the_reference_fixture(handle, f10):
    n = len(f10["hidx"])
    seen = set()
    for c in range(n):
        if f10["raises"][c]:
            continue
        h = int(f10["hidx"][c])
        H, g = f10[f"H_{h}"], f10[f"g_{h}"]
        seen.add(len(g))
        cond = float(f10["cond"][c])
        bound = max(1e-13, 2 * EPS * cond) if f10["group"][c] == 1 else 1e-13
        check_solve(handle, H, g, float(f10["M"][c]), float(f10["eps"][c]),
                    (f10[f"s_{c}"], int(f10["its"][c]), float(f10["lam"][c]), float(f10["dec"][c])), bound,
                    f"f10 case {c} group {int(f10['group'][c])}")
    assert {1, 63, 64, 65, 128} <= seen   # both ends and the edges of a row group


def test_dense_subproblem_matches_the_tridiagonal_fixture(handle, f3):
    for m in (3, 10, 50):
        for k in range(3):
            key = f"m{m}_k{k}"
            check_solve(handle, f3[f"{key}_T"], f3[f"{key}_g"], float(f3[f"{key}_M"]), 1e-8,
                        (f3[f"{key}_s"], int(f3[f"{key}_its"]), float(f3[f"{key}_r"]), float(f3[f"{key}_dec"])),
                        1e-13, f"f3 {key}")


def test_indefinite_block_is_status_1_and_zeros(handle, f10):
    c = int(np.flatnonzero(f10["raises"])[0])
    h = int(f10["hidx"][c])
    s, info = handle.cubic_dense(f10[f"H_{h}"], f10[f"g_{h}"], float(f10["M"][c]), r0=0.1, eps=float(f10["eps"][c]))
    assert info.solver_status == 1
    assert s.shape == (8,) and not s.any()


def test_it_max_returns_the_last_iterate(handle, f10):
    """root_scalar(method="newton") returns the last iterate without raising
    when maxiter runs out: status 3, the same root."""
    import warnings
    H, g, M = f10["H_2"], f10["g_2"], 5e-4
    s, info = handle.cubic_dense(H, g, M, r0=0.1, eps=1e-8, it_max=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s_ref, its, lam, dec = C.cubic_solver_root(g, H, M, it_max=2, epsilon=1e-8, r0=0.1)
    assert info.solver_status == 3 and info.solver_it == its == 2
    assert abs(info.lam - lam) <= 1e-13 * abs(lam)
    assert la_norm(s - s_ref) <= 1e-13 * la_norm(s_ref)


def test_argument_ranges_of_the_solver(handle):
    for k in (0, 129):
        with pytest.raises(_lib.KrcnError) as e:
            handle.cubic_dense(np.eye(k), np.ones(k), 1e-3)
        assert e.value.status == _lib.KRCN_ERR_INVALID
    with pytest.raises(_lib.KrcnError) as e:
        handle.cubic_dense(np.eye(2), np.ones(2), 1e-3, it_max=0)
    assert e.value.status == _lib.KRCN_ERR_INVALID


# ------------------------------------------------------------------ the step
def make_opt(A, b, device_step, k=10, reg_coef=1e-3, l2=0, dtype=torch.float64, window=0):
    loss = LogisticRegression(A, b, l1=0, l2=l2, store_mat_vec_prod=True, dtype=dtype)
    if window:
        loss.device_matrix.set_coord_window(window)
    return SSCN(loss=loss, reg_coef=reg_coef, label="SSCN", subspace_dim=k, tolerance=1e-9, tqdm=False,
                device_step=device_step)


def test_reference_trajectory_device_step(f6, f6_problem, monkeypatch):
    A, b = f6_problem

    def no_hvp(self, *a, **kw):
        raise AssertionError("SSCN called DeviceCSR.hvp")

    monkeypatch.setattr(krcn.DeviceCSR, "hvp", no_hvp)
    opt = make_opt(A, b, True)
    tr = opt.run(x0=np.full(A.shape[1], 0.5), it_max=6)
    assert opt.loss._cached(opt.x)
    assert opt.loss.value(opt.x) == opt.value
    opt.compute_loss_of_iterates()
    np.testing.assert_allclose(tr.loss_vals, f6["sscn_loss_vals"], rtol=1e-10)
    assert rel_err(np.asarray(tr.xs), f6["sscn_xs"]) < 1e-10
    its = np.diff(tr.solver_its)
    ref_its = np.diff(f6["sscn_solver_its"])
    assert len(its) == len(ref_its) and np.abs(its - ref_its).max() <= 1


def two_paths(A, b, steps, **kw):
    out = []
    for device_step in (False, True):
        opt = make_opt(A, b, device_step, **kw)
        opt.run(x0=np.full(A.shape[1], 0.5), it_max=steps)
        out.append(opt)
    return out


@pytest.mark.parametrize("l2", [0, 0.01])
@pytest.mark.parametrize("k", [1, 10, 120])
def test_device_step_vs_host_step(f7, k, l2):
    """The f7 problem (300 x 120, a dense and an empty column; k = 120 selects
    every column) with a 64-row window: three steps from the same seed."""
    A = golden_csr(f7).tocsc()
    host, dev = two_paths(A, f7["b"], 3, k=k, l2=l2, window=64)
    assert dev.it == host.it == 3
    assert dev.reg_coef == host.reg_coef
    assert rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy()) < 1e-10
    assert abs(dev.value - host.value) <= 1e-10 * abs(host.value)
    assert dev.loss._cached(dev.x)
    assert dev.loss.value(dev.x) == dev.value


def host_trials(opt, reg0):
    """Backtracking trials of the host path's last step from its reg_coef:
    reg0 * beta / beta ** trials, every factor a power of two."""
    t = np.log2(opt.reg_coef / (reg0 * opt.beta))
    assert t == round(t)
    return int(round(t))


@pytest.fixture(scope="module")
def backtracking(f6_problem):
    """The host path's first step from a reg_coef so small that the line search
    rejects trials beyond the second submission of the device step."""
    A, b = f6_problem
    reg0 = 1e-6
    opt = make_opt(A, b, False, reg_coef=reg0, l2=0.01)
    opt.run(x0=np.full(A.shape[1], 0.5), it_max=1)
    return reg0, opt


def test_backtracking_across_batch_boundaries(f6_problem, backtracking):
    A, b = f6_problem
    reg0, host = backtracking
    trials = host_trials(host, reg0)
    assert trials + 1 > FIRST_BATCH + BATCH
    assert trials < 20
    dev = make_opt(A, b, True, reg_coef=reg0, l2=0.01)
    dev.run(x0=np.full(A.shape[1], 0.5), it_max=1)
    assert dev.last_trials == trials
    assert dev.reg_coef == host.reg_coef
    assert rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy()) < 1e-10
    assert abs(dev.value - host.value) <= 1e-10 * abs(host.value)


def test_trial_cap_keeps_the_last_trial(f6_problem, backtracking):
    A, b = f6_problem
    reg0, host = backtracking
    assert host_trials(host, reg0) > 2
    l2 = 0.01
    loss = LogisticRegression(A, b, l1=0, l2=l2, store_mat_vec_prod=True)
    X = loss.device_matrix
    x = loss.to_device(np.full(A.shape[1], 0.5))
    value = loss.value(x)
    Ax = loss._device_Ax(x)
    I = np.random.default_rng(42).choice(A.shape[1], size=10, replace=False)
    x_new, Ax_new, info = X.sscn_step(I, x, loss._b_dev, value, reg0, Ax=Ax, l2=l2, max_trials=2)
    assert info.accepted == 0 and info.trials == 2
    M = reg0 * 0.5 / 0.5 / 0.5
    assert info.reg_coef == M
    # the second backtracking trial by the host pieces
    g = X.coord_gradient(I, Ax, loss._b_dev, x, l2)
    H = X.coord_hessian(I, Ax, l2)
    s, its, lam, dec = C.cubic_solver_root(g, H, M, r0=0.1, epsilon=EPS)
    want = x.clone()
    want[torch.from_numpy(I).to(x.device)] += torch.from_numpy(s).to(x.device)
    assert rel_err(x_new.cpu().numpy(), want.cpu().numpy()) < 1e-10
    assert rel_err(Ax_new.cpu().numpy(), X.coord_update(I, s, Ax).cpu().numpy()) < 1e-10
    assert abs(info.solver_it - its) <= 1
    assert abs(info.lam - lam) <= 1e-13 * abs(lam)
    assert abs(info.dx_norm - la_norm(s)) <= 1e-13 * la_norm(s)
    assert info.value_new > value - info.model_decrease
    assert info.lanczos.m_eff == 0 and info.lanczos.hvps == 0


def test_trial_cap_warns_and_is_counted(f6_problem):
    """A reg_coef so small that 20 doublings do not reach an accepted trial: the
    device step keeps the last trial, warns and counts the step."""
    A, b = f6_problem
    dev = make_opt(A, b, True, reg_coef=1e-12, l2=0.01)
    with pytest.warns(RuntimeWarning, match="no trial met the decrease test"):
        dev.run(x0=np.full(A.shape[1], 0.5), it_max=1)
    assert dev.capped_steps == 1 and dev.last_trials == 20
    assert dev.reg_coef == max(1e-12 * 0.5, EPS) * 2.0 ** 20
    host = make_opt(A, b, False, l2=0.01)
    host.run(x0=np.full(A.shape[1], 0.5), it_max=1)
    assert host.capped_steps == 0 and host.last_trials == host_trials(host, 1e-3)


def test_fp32_two_steps(f6_problem):
    """fp32 handle: the subproblem is fp64 on both paths and s is rounded to
    fp32 by the same expression in x + s, so the paths differ where the device
    solver's s differs from LAPACK's in its last fp64 bits.  The bounds are
    the margins the project's fp32 CRN test gives itself."""
    host, dev = two_paths(*f6_problem, 2, dtype=torch.float32)
    assert dev.reg_coef == host.reg_coef
    ex = rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy())
    ev = abs(dev.value - host.value) / abs(host.value)
    print(f"fp32 device step vs host path: x rel {ex:.3e}, value rel {ev:.3e}")
    assert ex < 1e-3
    assert ev < 1e-4


# ------------------------------------------------- refusals and allocation
def step_args(X, dtype=torch.float64):
    x = torch.full((X.d,), 0.5, dtype=dtype, device=X.device)
    bd = torch.zeros(X.n, dtype=dtype, device=X.device)
    return x, bd


def test_selection_refusals(handle):
    X = handle
    x, bd = step_args(X)
    with pytest.raises(_lib.KrcnError, match=r"cols_host\[3\] = 7 repeats cols_host\[1\]") as e:
        X.sscn_step([5, 7, 9, 7], x, bd, 0.7, 1e-3)
    assert e.value.status == _lib.KRCN_ERR_INVALID
    with pytest.raises(_lib.KrcnError, match=r"cols_host\[2\] = 120 outside") as e:
        X.sscn_step([5, 7, X.d], x, bd, 0.7, 1e-3)
    assert e.value.status == _lib.KRCN_ERR_INVALID
    big = krcn.DeviceCSR(synth.make_problem(None, seed=3, n=50, d=200, nnz=400)[0])
    xb, bb = step_args(big)
    with pytest.raises(_lib.KrcnError, match="k = 129") as e:
        big.sscn_step(np.arange(129), xb, bb, 0.7, 1e-3)
    assert e.value.status == _lib.KRCN_ERR_INVALID
    big.close()
    for kw in ({"max_trials": -1}, {"ls_beta": 1.0}, {"solver_it_max": 0}):
        with pytest.raises(_lib.KrcnError) as e:
            X.sscn_step([1, 2], x, bd, 0.7, 1e-3, **kw)
        assert e.value.status == _lib.KRCN_ERR_INVALID


def test_sharded_handle_is_unsupported(f7):
    X = krcn.DeviceCSR(golden_csr(f7), shard_mode=_lib.KRCN_SHARD_ROWS)
    x, bd = step_args(X)
    with pytest.raises(_lib.KrcnError) as e:
        X.sscn_step([1, 2], x, bd, 0.7, 1e-3)
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    X.close()


def test_repeated_steps_allocate_nothing(f7):
    A = golden_csr(f7)
    loss = LogisticRegression(A, f7["b"], l1=0, l2=0, store_mat_vec_prod=True)
    X = loss.device_matrix
    x = loss.to_device(f7["x"])
    value = loss.value(x)
    sizes = []
    for seed in range(3):
        I = np.random.default_rng(seed).choice(X.d, size=10, replace=False)
        X.sscn_step(I, x, loss._b_dev, value, 1e-3, Ax=loss._device_Ax(x))
        sizes.append(X.owned_bytes())
    assert sizes[0] == sizes[1] == sizes[2]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_first_call_without_Ax_builds_the_plans_first(f6_problem, dtype):
    """Ax=None as the first compute call of a fresh handle with two placements
    probed and the second kept: the plan build inside the call relocates the
    scratch vectors and the partials, and the step must read them afterwards.
    Against the same step with Ax supplied on a handle without the probe."""
    A, b = f6_problem
    loss = LogisticRegression(A, b, l1=0, l2=0.01, store_mat_vec_prod=True, dtype=dtype)
    x = loss.to_device(np.full(A.shape[1], 0.5))
    value = loss.value(x)
    I = np.random.default_rng(7).choice(A.shape[1], size=10, replace=False)
    Acsr = A.tocsr()
    Y = krcn.DeviceCSR(Acsr, dtype=dtype)
    Y.set_placement_trials(0)
    want = Y.sscn_step(I, x, loss._b_dev, value, 1e-3, Ax=Y.matvec(x), l2=0.01)
    Y.close()
    X = krcn.DeviceCSR(Acsr, dtype=dtype)
    X.set_placement_trials(2)
    X.set_placement_keep(1)
    # (nothing before the step may build the plans: placement_info would)
    for call in ("first", "second"):
        got = X.sscn_step(I, x, loss._b_dev, value, 1e-3, l2=0.01)
        info = X.placement_info()
        assert info["probed"] == 2 and info["kept"] == 1, call
        for name, a, w in (("x_new", got[0], want[0]), ("Ax_new", got[1], want[1])):
            assert torch.equal(a, w), f"{call} call: {name}"
        for field in ("accepted", "trials", "solver_it", "solver_status", "reg_coef", "lam", "model_decrease",
                      "value_new", "dx_norm"):
            assert getattr(got[2], field) == getattr(want[2], field), f"{call} call: {field}"
    X.close()


def test_matrix_without_rows_is_the_l2_model():
    """n == 0: no loss terms, so f = l2 / 2 ||x||^2, the gradient l2 x_I and the Hessian l2 I."""
    import scipy.sparse as sp
    l2 = 0.5
    X = krcn.DeviceCSR(sp.csr_matrix((0, 9)))
    x = torch.linspace(-1.0, 1.0, 9, dtype=torch.float64, device=X.device)
    none = torch.empty(0, dtype=torch.float64, device=X.device)
    xh = x.cpu().numpy()
    value = l2 / 2 * float(np.linalg.norm(xh)) ** 2
    I = np.array([8, 0, 3])
    for Ax in (None, none):
        x_new, Ax_new, info = X.sscn_step(I, x, none, value, 1e-3, Ax=Ax, l2=l2)
        s, its, lam, dec = C.cubic_solver_root(l2 * xh[I], l2 * np.eye(3), info.reg_coef, r0=0.1, epsilon=EPS)
        want = xh.copy()
        want[I] += s
        assert info.accepted == 1 and info.solver_status == 0
        assert rel_err(x_new.cpu().numpy(), want) < 1e-13
        assert Ax_new.numel() == 0
        assert np.isfinite(info.value_new)
        nrm = X.diff_norm(x_new)
        assert info.value_new == l2 / 2 * (nrm * nrm)
        assert info.value_new <= value - info.model_decrease
    X.close()


def test_empty_matrix_is_the_l2_model():
    """nnz == 0: the gradient is l2 x_I, the Hessian l2 I and Ax_new a copy of Ax."""
    import scipy.sparse as sp
    l2 = 0.5
    X = krcn.DeviceCSR(sp.csr_matrix((6, 9)))
    x = torch.linspace(-1.0, 1.0, 9, dtype=torch.float64, device=X.device)
    bd = torch.zeros(6, dtype=torch.float64, device=X.device)
    Ax = torch.zeros(6, dtype=torch.float64, device=X.device)
    value = float(np.log(2.0) + l2 / 2 * float((x * x).sum()))
    I = np.array([8, 0, 3])
    x_new, Ax_new, info = X.sscn_step(I, x, bd, value, 1e-3, Ax=Ax, l2=l2)
    xh = x.cpu().numpy()
    s, its, lam, dec = C.cubic_solver_root(l2 * xh[I], l2 * np.eye(3), info.reg_coef, r0=0.1, epsilon=EPS)
    want = xh.copy()
    want[I] += s
    assert info.accepted == 1
    assert rel_err(x_new.cpu().numpy(), want) < 1e-13
    assert not Ax_new.cpu().numpy().any()
    X.close()
