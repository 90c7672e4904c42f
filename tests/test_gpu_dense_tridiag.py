"""The dense cubic subproblem and SSCN's device step over one tridiagonal
reduction (krcn_dense_tridiag, krcn_cubic_dense_tridiag, krcn_sscn_step_tridiag)
against the same route on the CPU, the reference's outputs and the host path.

The reduction.  The yardstick of every figure is the same figure of the CPU
route on the same input: g's Householder reflector, then
scipy.linalg.hessenberg.  The device may be at most 4 x that, or K eps (K = k + 1)
where the CPU figure is smaller: an entry of Q^T Q is a sum of K rounded
products, and both are backward-stable Householder reductions whose constants
differ with the summation order, not with the method.

The subproblem.  s (relative 2-norm), lam and the model decrease within
max(1e-13, 4 e_cpu) of the reference's cubic_solver_root (the fixtures f10 and
f11 for k <= 129, its dense branch run here for k = 257, 500, 1000), where
e_cpu is the error of the CPU route (hessenberg, then
cubic_solver_root_tridiag) on the same case — one figure a case, the largest of
its three errors — and 1e-13 the project's floor for the dense kernel; Newton
iteration counts within one of the reference's.  (Quantity by quantity the
bound would be a ratio of two rounding errors of the same size, each measured
against a reference that carries a third: on f10's case 48, k = 16 with
cond(H + lam I) of 6e4, the device's lam is 3.4e-12 off the reference and the
CPU route's 6.6e-13, while their s are 5.6e-12 and 4.5e-12 off; case 49, the
same block at the other xtol, is the one other such case.  Per case the largest
device error measured is 1.6 x e_cpu.)

The step.  fp64 trajectories at the project's 1e-10 with equal trial counts;
fp32 within 4 fp32 ulps of the host path at each entry's magnitude (s agrees
to ~1e-15, the cast and the add round once each).

Rows per workgroup of a column launch: kSytdR = 4, one per wave of w = 4, so
R w = 16; the prologue's loops stride the 256 threads of the workgroup.
"""
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import torch

import krcn
from conftest import PKG, golden_csr, load_golden, rel_err
from krcn import _lib, synth
from optimizer import cubic as C
from optimizer.cubic import SSCN
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)


def rows_per_workgroup():
    text = open(os.path.join(PKG, "csrc", "krcn_sytd.hpp")).read()
    return int(re.search(r"constexpr int kSytdR = (\d+);", text).group(1))


R = rows_per_workgroup()
RW = R * 4


@pytest.fixture(scope="module")
def handle():
    X = krcn.DeviceCSR(sp.random(40, 30, density=0.2, random_state=1, format="csr"))
    yield X
    X.close()


# ---------------------------------------------------------------- the CPU route
def mirrored(H):
    """The matrix the calls see: the upper triangle, mirrored."""
    U = np.triu(np.asarray(H, dtype=np.float64))
    return U + np.triu(U, 1).T


def g_reflector(g):
    """dlarfg on g: (P0, b0) with P0 g = b0 e1, P0 = I when g[1:] is zero."""
    k = len(g)
    xn = float(np.linalg.norm(g[1:])) if k > 1 else 0.0
    if xn == 0.0:
        return np.eye(k), float(g[0])
    b0 = -np.copysign(np.hypot(g[0], xn), g[0])
    tau = (b0 - g[0]) / b0
    v = np.concatenate(([1.0], g[1:] / (g[0] - b0)))
    return np.eye(k) - tau * np.outer(v, v), float(b0)


def cpu_tridiag(H, g):
    """(alphas, off-diagonal, b0, Q) by g's reflector and scipy.linalg.hessenberg."""
    P0, b0 = g_reflector(np.asarray(g, dtype=np.float64))
    H1 = P0 @ H @ P0
    H1 = (H1 + H1.T) / 2
    if len(g) > 2:
        Hh, Qh = sla.hessenberg(H1, calc_q=True)
    else:
        Hh, Qh = H1, np.eye(len(g))
    return np.diag(Hh).copy(), np.diag(Hh, -1).copy(), b0, P0 @ Qh


def figures(H, g, al, off, b0, Q):
    k = len(g)
    T = np.diag(al) + np.diag(off, 1) + np.diag(off, -1)
    hn = float(np.linalg.norm(H))
    orth = float(np.abs(Q.T @ Q - np.eye(k)).max())
    recon = float(np.linalg.norm(Q @ T @ Q.T - H)) / (hn if hn else 1.0)
    first = float(np.abs(Q[:, 0] * b0 - g).max()) / (abs(b0) if b0 else 1.0)
    if b0 == 0.0:
        first = float(np.abs(Q[:, 0] - np.eye(k)[:, 0]).max())
    ev = sla.eigvalsh_tridiagonal(al, off) if k > 1 else al.copy()
    eh = np.linalg.eigvalsh(H)
    scale = float(np.abs(eh).max())
    eig = float(np.abs(np.sort(ev) - eh).max()) / (scale if scale else 1.0)
    return dict(orth=orth, recon=recon, first=first, eig=eig)


RATIOS = []   # (label, figure, device, cpu) of every reduction checked, for the record


def check_reduction(X, H, g, label):
    k = len(g)
    Hm = mirrored(H)
    al, be, Q = X.dense_tridiag(H, g, want_q=True)
    assert np.isfinite(al).all() and np.isfinite(be).all() and np.isfinite(Q).all()
    al2, be2, Q2 = X.dense_tridiag(H, g, want_q=True)
    assert al.tobytes() == al2.tobytes() and be.tobytes() == be2.tobytes() and Q.tobytes() == Q2.tobytes()
    dev = figures(Hm, g, al, be[1:], float(be[0]), Q)
    cpu = figures(Hm, g, *cpu_tridiag(Hm, g))
    assert abs(abs(be[0]) - float(np.linalg.norm(g))) <= 4 * EPS * float(np.linalg.norm(g))
    for name in ("orth", "recon", "first", "eig"):
        bound = max(4 * cpu[name], (k + 1) * EPS)
        RATIOS.append((label, name, dev[name], cpu[name]))
        print(f"{label}: k {k} {name} device {dev[name]:.3e} cpu {cpu[name]:.3e} "
              f"ratio {dev[name] / cpu[name] if cpu[name] else float('inf'):.2f} bound {bound:.3e}")
    for name in ("orth", "recon", "first", "eig"):
        assert dev[name] <= max(4 * cpu[name], (k + 1) * EPS), (label, name, dev[name], cpu[name])
    return al, be, Q


def logistic_block(k, seed, n=1500):
    """A coordinate Hessian and gradient of a synthetic logistic problem over k columns."""
    rng = np.random.default_rng(seed)
    A = sp.random(n, k, density=min(1.0, 12.0 / k + 0.01), random_state=seed, format="csr").toarray()
    x = rng.standard_normal(k) * 0.3
    b = (rng.random(n) < 0.5).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-(A @ x)))
    H = A.T @ ((p * (1 - p))[:, None] * A) / n
    return (H + H.T) / 2, A.T @ (p - b) / n


SIZES = [1, 2, 3, RW - 1, RW, RW + 1, 63, 64, 65, 128, 129, 255, 256, 257, 1024]


@pytest.mark.parametrize("k", SIZES)
def test_reduction_of_a_coordinate_hessian(handle, k):
    H, g = logistic_block(k, seed=100 + k)
    check_reduction(handle, H, g, "hessian")


@pytest.mark.parametrize("k", [3, RW + 1, 65, 129, 300])
def test_reduction_of_the_degenerate_inputs(handle, k):
    rng = np.random.default_rng(k)
    H, g = logistic_block(k, seed=200 + k)
    # a diagonal H under a general g, and under g = c e_1, where every tau is zero
    D = np.diag(rng.uniform(0.1, 2.0, k))
    al, be, Q = check_reduction(handle, D, g, "diagonal")
    g1 = np.zeros(k)
    g1[0] = 0.3
    al, be, Q = check_reduction(handle, D, g1, "diagonal, g = c e_1")
    assert np.array_equal(al, np.diag(D)) and be[0] == 0.3 and not be[1:].any() and np.array_equal(Q, np.eye(k))
    # g = 0: no first reflector either, b_0 = 0 and Q e1 = e1
    al, be, Q = check_reduction(handle, H, np.zeros(k), "g = 0")
    assert be[0] == 0.0
    # g a multiple of e_3
    ge = np.zeros(k)
    ge[2] = -0.7
    al, be, Q = check_reduction(handle, H, ge, "g = c e_3")
    assert abs(be[0]) == 0.7
    # a block-diagonal H whose second block g does not reach: a zero b mid-way
    m1 = k // 2 + 1
    Hb = np.zeros((k, k))
    Hb[:m1, :m1] = H[:m1, :m1]
    Hb[m1:, m1:] = H[m1:, m1:] + np.eye(k - m1)
    gb = g.copy()
    gb[m1:] = 0.0
    al, be, Q = check_reduction(handle, Hb, gb, "two blocks")
    assert be[m1] == 0.0
    # only the upper triangle may be read
    Hn = H.copy()
    Hn[np.tril_indices(k, -1)] = np.nan
    aln, ben, Qn = handle.dense_tridiag(Hn, g, want_q=True)
    al, be, Q = handle.dense_tridiag(H, g, want_q=True)
    assert aln.tobytes() == al.tobytes() and ben.tobytes() == be.tobytes() and Qn.tobytes() == Q.tobytes()


def test_diagonal_h_and_zero_g_at_the_largest_block(handle):
    k = 1024
    D = np.diag(np.linspace(0.5, 3.0, k))
    al, be, Q = handle.dense_tridiag(D, np.zeros(k), want_q=True)
    assert np.array_equal(al, np.diag(D)) and not be.any() and np.array_equal(Q, np.eye(k))


# ------------------------------------------------------------ the subproblem
def la_norm(v):
    return float(np.linalg.norm(np.asarray(v, dtype=np.float64)))


def errors(got, ref):
    s, lam, dec = got
    s_ref, lam_ref, dec_ref = ref
    return (la_norm(s - s_ref) / la_norm(s_ref), abs(lam - lam_ref) / abs(lam_ref), abs(dec - dec_ref) / abs(dec_ref))


def cpu_route(H, g, M, eps):
    al, off, b0, Q = cpu_tridiag(H, g)
    gT = np.zeros(len(g))
    gT[0] = b0
    sT, its, lam, dec = C.cubic_solver_root_tridiag(gT, al, off, M, epsilon=eps, r0=0.1)
    return Q @ sT, its, lam, dec


WORST = {}   # the largest device error seen, its e_cpu and the iteration-count differences


def check_solve(X, H, g, M, eps, ref, label):
    s_ref, its, lam, dec = ref
    Hm = mirrored(H)
    cs, cits, clam, cdec = cpu_route(Hm, g, M, eps)
    e_cpu = errors((cs, clam, cdec), (s_ref, lam, dec))
    s, info = X.cubic_dense_tridiag(H, g, M, r0=0.1, eps=eps)
    assert np.isfinite(s).all()
    e_dev = errors((s, info.lam, info.model_decrease), (s_ref, lam, dec))
    print(f"{label}: k {len(g)} M {M:g} eps {eps:g} its {info.solver_it}/{its} (cpu route {cits}) "
          f"device s {e_dev[0]:.2e} lam {e_dev[1]:.2e} dec {e_dev[2]:.2e} | "
          f"e_cpu s {e_cpu[0]:.2e} lam {e_cpu[1]:.2e} dec {e_cpu[2]:.2e}")
    w = WORST.setdefault("err", (0.0, 0.0, ""))
    if max(e_dev) > w[0]:
        WORST["err"] = (max(e_dev), e_cpu[int(np.argmax(e_dev))], label)
    WORST.setdefault("its", set()).add(info.solver_it - its)
    assert info.solver_status == 0
    assert info.reg_coef == M
    bound = max(1e-13, 4 * max(e_cpu))   # one e_cpu a case: the CPU route's largest error on it
    for ed in e_dev:
        assert ed <= bound
    assert abs(info.solver_it - its) <= 1


def fixture_cases(f):
    for c in range(len(f["hidx"])):
        if f["raises"][c]:
            continue
        h = int(f["hidx"][c])
        yield c, f[f"H_{h}"], f[f"g_{h}"], float(f["M"][c]), float(f["eps"][c]), (
            f[f"s_{c}"], int(f["its"][c]), float(f["lam"][c]), float(f["dec"][c]))


def test_subproblem_matches_the_reference_fixture_up_to_128(handle):
    f10 = load_golden("f10_cubic_dense.npz")
    seen = set()
    for c, H, g, M, eps, ref in fixture_cases(f10):
        seen.add(len(g))
        check_solve(handle, H, g, M, eps, ref, f"f10 case {c} group {int(f10['group'][c])}")
    assert {1, 2, 63, 64, 65, 128} <= seen


def test_subproblem_matches_the_reference_fixture_at_129(handle):
    f11 = load_golden("f11_cubic_dense_tridiag.npz")
    n = 0
    for c, H, g, M, eps, ref in fixture_cases(f11):
        assert len(g) == 129 and M in (1e-3, 1.0) and eps in (1e-8, EPS)
        check_solve(handle, H, g, M, eps, ref, f"f11 case {c} group {int(f11['group'][c])}")
        n += 1
    assert n == 8


@pytest.mark.parametrize("k", [257, 500, 1000])
def test_subproblem_matches_the_dense_branch_above_the_fixtures(handle, k):
    H, g = logistic_block(k, seed=300 + k)
    for M in (1e-3, 1.0):
        for eps in (1e-8, EPS):
            ref = C.cubic_solver_root(g, H, M, epsilon=eps, r0=0.1)   # a dense H: the dense branch
            check_solve(handle, H, g, M, eps, ref, "dense branch")
    print("worst so far:", WORST)


def test_negative_definite_block_is_status_1_and_zeros(handle):
    f10 = load_golden("f10_cubic_dense.npz")
    c = int(np.flatnonzero(f10["raises"])[0])
    h = int(f10["hidx"][c])
    s, info = handle.cubic_dense_tridiag(f10[f"H_{h}"], f10[f"g_{h}"], float(f10["M"][c]), r0=0.1,
                                         eps=float(f10["eps"][c]))
    assert info.solver_status == 1
    assert s.shape == (8,) and not s.any()
    k = 200
    rng = np.random.default_rng(5)
    Bm = rng.standard_normal((k, k))
    H = -(Bm @ Bm.T / k + np.eye(k))
    s, info = handle.cubic_dense_tridiag(H, rng.standard_normal(k), 1e-6, r0=0.1, eps=1e-8)
    assert info.solver_status == 1
    assert s.shape == (k,) and not s.any()


def test_argument_ranges_of_the_solver(handle):
    for k in (0, 1025):
        with pytest.raises(_lib.KrcnError) as e:
            handle.cubic_dense_tridiag(np.eye(k), np.ones(k), 1e-3)
        assert e.value.status == _lib.KRCN_ERR_INVALID
        with pytest.raises(_lib.KrcnError) as e:
            handle.dense_tridiag(np.eye(k), np.ones(k))
        assert e.value.status == _lib.KRCN_ERR_INVALID
    with pytest.raises(_lib.KrcnError) as e:
        handle.cubic_dense_tridiag(np.eye(2), np.ones(2), 1e-3, it_max=0)
    assert e.value.status == _lib.KRCN_ERR_INVALID
    # the Cholesky route keeps its cap
    with pytest.raises(_lib.KrcnError) as e:
        handle.cubic_dense(np.eye(129), np.ones(129), 1e-3)
    assert e.value.status == _lib.KRCN_ERR_INVALID


# ------------------------------------------------------------------ the step
@pytest.fixture(scope="module")
def problem():
    A, b = synth.make_problem(None, seed=11, n=300, d=400, nnz=6000)
    return A.tocsc(), b


def make_opt(A, b, device_step, k, subproblem="cholesky", reg_coef=1e-3, l2=0, dtype=torch.float64):
    loss = LogisticRegression(A, b, l1=0, l2=l2, store_mat_vec_prod=True, dtype=dtype)
    return SSCN(loss=loss, reg_coef=reg_coef, label="SSCN", subspace_dim=k, tolerance=1e-9, tqdm=False,
                device_step=device_step, subproblem=subproblem)


def run_steps(opt, steps):
    """The trial counts of `steps` steps from x = 0.5."""
    trials, step = [], opt.step

    def recording_step():
        step()
        trials.append(opt.last_trials)

    opt.step = recording_step
    opt.run(x0=np.full(opt.loss.dim, 0.5), it_max=steps)
    return trials


def assert_same_trajectory(dev, host, td, th):
    assert td == th and len(td) == 3
    assert dev.reg_coef == host.reg_coef
    ex = rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy())
    ev = abs(dev.value - host.value) / abs(host.value)
    print(f"k {dev.subspace_dim}: trials {td}, x rel {ex:.3e}, value rel {ev:.3e}")
    assert ex < 1e-10
    assert ev <= 1e-10
    assert dev.loss._cached(dev.x)
    assert dev.loss.value(dev.x) == dev.value


@pytest.mark.parametrize("l2", [0, 0.01])
@pytest.mark.parametrize("k", [150, 400])
def test_tridiag_step_vs_host_step(problem, k, l2):
    """n = 300, d = 400 (k = 400 selects every column): three steps from the same seed."""
    A, b = problem
    host = make_opt(A, b, False, k, l2=l2)
    th = run_steps(host, 3)
    dev = make_opt(A, b, True, k, subproblem="tridiag", l2=l2)
    td = run_steps(dev, 3)
    assert_same_trajectory(dev, host, td, th)


@pytest.mark.parametrize("l2", [0, 0.01])
def test_tridiag_step_vs_cholesky_step(problem, l2):
    A, b = problem
    chol = make_opt(A, b, True, 100, l2=l2)
    tc = run_steps(chol, 3)
    tri = make_opt(A, b, True, 100, subproblem="tridiag", l2=l2)
    tt = run_steps(tri, 3)
    assert_same_trajectory(tri, chol, tt, tc)


def test_backtracking_reuses_the_one_reduction():
    """The f6 problem from a reg_coef so small that the line search rejects trials
    beyond the second submission (tests/test_gpu_sscn_step.py's case): every trial
    solves over the reduction the step made before the first."""
    f6 = load_golden("f6_methods.npz")
    n, d, nnz = (int(v) for v in f6["shape"])
    A, b = synth.make_problem(None, seed=int(f6["seed"]), n=n, d=d, nnz=nnz)
    A = A.tocsc()
    host = make_opt(A, b, False, 10, reg_coef=1e-6, l2=0.01)
    th = run_steps(host, 1)
    dev = make_opt(A, b, True, 10, subproblem="tridiag", reg_coef=1e-6, l2=0.01)
    td = run_steps(dev, 1)
    print(f"backtracking trials: host {th}, device {td}")
    assert th[0] + 1 > 2 + 4 and th[0] < 20   # past the first two submissions, under the cap
    assert td == th
    assert dev.reg_coef == host.reg_coef
    assert rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy()) < 1e-10
    assert abs(dev.value - host.value) <= 1e-10 * abs(host.value)


def test_fp32_two_steps(problem):
    """x within 4 fp32 ulps of the host path at each entry's magnitude."""
    A, b = problem
    host = make_opt(A, b, False, 150, dtype=torch.float32)
    th = run_steps(host, 2)
    dev = make_opt(A, b, True, 150, subproblem="tridiag", dtype=torch.float32)
    td = run_steps(dev, 2)
    assert td == th and dev.reg_coef == host.reg_coef
    xd, xh = dev.x.cpu().numpy(), host.x.cpu().numpy()
    assert xd.dtype == np.float32
    ulps = np.abs(xd.astype(np.float64) - xh.astype(np.float64)) / np.spacing(np.abs(xh)).astype(np.float64)
    print(f"fp32 tridiag step vs host path: largest difference {ulps.max():.2f} ulps, "
          f"{int((ulps > 0).sum())} of {len(ulps)} entries differ")
    assert ulps.max() <= 4


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_first_call_without_Ax_builds_the_plans_first(problem, dtype):
    """Ax=None as the first compute call of a fresh handle with two placements
    probed and the second kept, against the same step with Ax supplied on a
    handle without the probe: bitwise."""
    A, b = problem
    loss = LogisticRegression(A, b, l1=0, l2=0.01, store_mat_vec_prod=True, dtype=dtype)
    x = loss.to_device(np.full(A.shape[1], 0.5))
    value = loss.value(x)
    I = np.random.default_rng(7).choice(A.shape[1], size=150, replace=False)
    Acsr = A.tocsr()
    Y = krcn.DeviceCSR(Acsr, dtype=dtype)
    Y.set_placement_trials(0)
    want = Y.sscn_step(I, x, loss._b_dev, value, 1e-3, Ax=Y.matvec(x), l2=0.01, subproblem="tridiag")
    Y.close()
    X = krcn.DeviceCSR(Acsr, dtype=dtype)
    X.set_placement_trials(2)
    X.set_placement_keep(1)
    # (nothing before the step may build the plans: placement_info would)
    for call in ("first", "second"):
        got = X.sscn_step(I, x, loss._b_dev, value, 1e-3, l2=0.01, subproblem="tridiag")
        info = X.placement_info()
        assert info["probed"] == 2 and info["kept"] == 1, call
        for name, a, w in (("x_new", got[0], want[0]), ("Ax_new", got[1], want[1])):
            assert torch.equal(a, w), f"{call} call: {name}"
        for field in ("accepted", "trials", "solver_it", "solver_status", "reg_coef", "lam", "model_decrease",
                      "value_new", "dx_norm"):
            assert getattr(got[2], field) == getattr(want[2], field), f"{call} call: {field}"
    X.close()


def step_args(X, dtype=torch.float64):
    x = torch.full((X.d,), 0.5, dtype=dtype, device=X.device)
    bd = torch.zeros(X.n, dtype=dtype, device=X.device)
    return x, bd


def test_selection_refusals(problem):
    A, b = problem
    X = krcn.DeviceCSR(A.tocsr())
    x, bd = step_args(X)
    with pytest.raises(_lib.KrcnError, match=r"cols_host\[3\] = 7 repeats cols_host\[1\]") as e:
        X.sscn_step([5, 7, 9, 7], x, bd, 0.7, 1e-3, subproblem="tridiag")
    assert e.value.status == _lib.KRCN_ERR_INVALID
    with pytest.raises(_lib.KrcnError, match=r"cols_host\[2\] = 400 outside") as e:
        X.sscn_step([5, 7, X.d], x, bd, 0.7, 1e-3, subproblem="tridiag")
    assert e.value.status == _lib.KRCN_ERR_INVALID
    # the existing step still refuses one column past its cap
    with pytest.raises(_lib.KrcnError, match="k = 129") as e:
        X.sscn_step(np.arange(129), x, bd, 0.7, 1e-3)
    assert e.value.status == _lib.KRCN_ERR_INVALID
    with pytest.raises(ValueError, match="subproblem"):
        X.sscn_step([1, 2], x, bd, 0.7, 1e-3, subproblem="lanczos")
    X.close()
    big = krcn.DeviceCSR(synth.make_problem(None, seed=3, n=50, d=1100, nnz=2000)[0])
    xb, bb = step_args(big)
    with pytest.raises(_lib.KrcnError, match="k = 1025") as e:
        big.sscn_step(np.arange(1025), xb, bb, 0.7, 1e-3, subproblem="tridiag")
    assert e.value.status == _lib.KRCN_ERR_INVALID
    big.close()


def test_sharded_handle_is_unsupported(problem):
    A, b = problem
    X = krcn.DeviceCSR(A.tocsr(), shard_mode=_lib.KRCN_SHARD_ROWS)
    x, bd = step_args(X)
    with pytest.raises(_lib.KrcnError) as e:
        X.sscn_step([1, 2], x, bd, 0.7, 1e-3, subproblem="tridiag")
    assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    X.close()


def test_workspace_is_allocated_once_and_counted(problem):
    A, b = problem
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    X = loss.device_matrix
    x = loss.to_device(np.full(A.shape[1], 0.5))
    value = loss.value(x)
    k = 150
    launches, ws = krcn.DeviceCSR.dense_tridiag_geometry(k)
    assert launches == k - 1
    # the coordinate workspace and the chain state are the existing step's: take them first
    I = np.random.default_rng(0).choice(X.d, size=k, replace=False)
    X.coord_hessian(I, loss._device_Ax(x))
    X.sscn_step(I[:10], x, loss._b_dev, value, 1e-3, Ax=loss._device_Ax(x))
    before = X.owned_bytes()
    sizes = []
    for seed in range(3):
        I = np.random.default_rng(seed).choice(X.d, size=k, replace=False)
        X.sscn_step(I, x, loss._b_dev, value, 1e-3, Ax=loss._device_Ax(x), subproblem="tridiag")
        sizes.append(X.owned_bytes())
    assert sizes[0] - before == ws
    assert sizes[0] == sizes[1] == sizes[2]
