"""The batched Krylov-CRN step (krcn_crn_step_block, Cubic_Krylov_LS_Batch) and
its pieces (krcn_gradient_block, krcn_value_block, krcn_cubic_tridiag_block).

Expectations come from oracle/krcn_oracle.py (`oracle_steps` below restates its
krylov_crn with the per-trial quantities kept) and from the single device step
(Cubic_Krylov_LS(device_step=True)) on each column's problem.

Tolerances are the project's own: gradient 1e-13 and value 1e-12 against the
oracle (the loss terms are non-negative, so any summation order agrees within
n 2^-53 = 2.2e-13 at n = 2,000); x and values against the single device step and
the oracle 1e-10, as tests/test_gpu_crn_step.py uses between its two paths; fp32
the bounds of its test_fp32_two_steps (1e-3 on x, 1e-4 on values).

The cases (test_cases_are_what_they_claim recomputes all of this on the CPU):
the f4 problem at x0 = 0.5, m = 10, six columns (labels, l2, reg_coef); over
three steps all accept at trial 0 except the fifth, which needs 16 trials in its
first step (past the first and the second submission); every decision margin
|value_new - (value - model_decrease)| / |value| is >= 1.5e-3 and every beta
>= 1.7e-4; the 300 x 6 breakdown matrix gives m_eff = 6 with breaking betas of
1e-15 .. 8e-15 and kept betas >= 2e-4.
"""
import numpy as np
import numpy.linalg as la
import pytest
import torch

import krcn
import krcn_oracle as O
from conftest import rel_err
from krcn import _lib, synth
from optimizer.cubic import Cubic_Krylov_LS, Cubic_Krylov_LS_Batch
from optimizer.loss import LogisticRegression

gpu = pytest.mark.gpu
DEV = "cuda"
M = 10


def t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def h(x):
    return x.detach().cpu().numpy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the cases
class Cases:
    def __init__(self):
        self.A, self.b = synth.make_problem(None, seed=99, n=2000, d=5000, nnz=60_000)
        n = self.A.shape[0]
        b01 = O.labels01(self.b)
        flip = np.random.default_rng(3).random(n) < 0.3
        bf = np.where(flip, 1 - b01, b01)
        # (0/1 labels, l2, reg_coef)
        self.cols = [(b01, 0.0, 1e-3), (b01, 0.01, 1e-3), (1 - b01, 0.0, 1e-3), (bf, 0.001, 1e-2),
                     (b01, 0.0, 1e-9), (b01, 0.0, 10.0)]
        self.x0 = np.full(self.A.shape[1], 0.5)
        self.Ab, self.bb = synth.make_problem(None, seed=5, n=300, d=6, nnz=900)
        bb01 = O.labels01(self.bb)
        self.bcols = [(bb01, 0.0, 1e-3), (bb01, 0.01, 1e-3), (1 - bb01, 0.0, 1e-2)]
        self._ref = {}

    def B(self, cols):
        return np.stack([c[0] for c in cols], axis=1)

    def ref(self, which, c, steps, m=M):
        key = (which, c, steps, m)
        if key not in self._ref:
            A, cols = (self.A, self.cols) if which == "f4" else (self.Ab, self.bcols)
            b01, l2, reg = cols[c]
            self._ref[key] = oracle_steps(A, b01, np.full(A.shape[1], 0.5), m, reg, l2, steps)
        return self._ref[key]


def oracle_steps(A, b01, x0, m, reg_coef, l2, steps, beta=0.5):
    """O.krylov_crn's loop (cubic.py:265-309) from the oracle's pieces, keeping per
    step the trial count, the decision margins and the recurrence's betas."""
    x = np.array(x0, dtype=np.float64)
    fval = O.value(A, b01, x, l2)
    r0, solver_it, out = 0.1, 0, []
    for _ in range(steps):
        g = O.gradient(A, b01, x, l2)
        w = O.hessian_weights(A, x)
        V, alphas, betas, beta_last = O.lanczos(lambda v: O.hvp_from_weights(A, w, v, l2), g, m)
        T = np.diag(alphas) + np.diag(betas, -1) + np.diag(betas, 1)
        gs = np.zeros(len(alphas))
        gs[0] = la.norm(g)
        rc, trials, margins = reg_coef * beta, 0, []
        while True:
            s, its, r0_new, dec = O.cubic_solver_root(gs, T, rc, epsilon=1e-8, r0=r0)
            x_new = x + V @ s
            f_new = O.value(A, b01, x_new, l2)
            margins.append(abs(f_new - (fval - dec)) / abs(fval))
            if not (f_new > fval - dec and trials < 20):
                break
            rc, trials = rc / beta, trials + 1
        solver_it += its
        out.append(dict(x_old=x, x=x_new, value=f_new, reg_coef=rc, r0=r0_new, solver_it=solver_it, its=its,
                        m_eff=len(alphas), trials=trials, margins=margins, betas=betas, beta_last=beta_last,
                        accepted=not f_new > fval - dec))
        x, reg_coef, fval, r0 = x_new, rc, f_new, r0_new
    return out


@pytest.fixture(scope="module")
def cases():
    return Cases()


def test_cases_are_what_they_claim(cases):
    for c in range(6):
        ref = cases.ref("f4", c, 3)
        want = [16, 0, 0] if c == 4 else [0, 0, 0]
        assert [s["trials"] for s in ref] == want, c
        for s in ref:
            assert s["accepted"] and s["m_eff"] == M
            assert min(s["margins"]) > 1e-6          # measured: >= 1.5e-3
            assert s["betas"].min() > 1e-5           # measured: >= 1.7e-4
    # the restated loop is the oracle's
    b01, l2, reg = cases.cols[1]
    kc = O.krylov_crn(cases.A, b01, cases.x0, m=M, reg_coef=reg, it_max=3, l2=l2)
    ref = cases.ref("f4", 1, 3)
    assert np.array_equal(kc["xs"][-1], ref[-1]["x"]) and kc["value"][-1] == ref[-1]["value"]
    assert list(kc["solver_it"]) == [s["solver_it"] for s in ref]
    # a 16-trial chain crosses the first (2 trials) and the second (4 more) submission
    assert 16 + 1 > 2 + 4
    for c in range(3):
        for m in (10, 7):
            s = cases.ref("brk", c, 1, m)[0]
            assert s["m_eff"] == (6 if m == 10 else 7)
            assert abs(s["beta_last"]) < 1e-9        # measured: 1e-15 .. 8e-15
            kept = s["betas"][:5]
            assert kept.min() > 1e-5                 # measured: >= 2e-4
            if m == 7:
                assert s["betas"][5] == 0.0          # j_break = m - 2: seven vectors, the last zero
            assert s["trials"] == 0 and min(s["margins"]) > 1e-6   # measured: >= 3.7e-2


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def X(cases):
    Xd = krcn.DeviceCSR(cases.A)
    yield Xd
    Xd.close()


def start(cases, X, cols, dtype=torch.float64):
    """The (d, k) start block, X xs, the label block and the start values of a batch."""
    k = len(cols)
    xs = t(np.repeat(cases.x0[:, None], k, axis=1), dtype)
    AX = X.matvec_block(xs)
    B = t(cases.B(cols), dtype)
    l2 = np.array([c[1] for c in cols])
    reg = np.array([c[2] for c in cols])
    return xs, AX, B, l2, reg, X.value_block(AX, B, xs, l2)


@pytest.fixture(scope="module")
def mixed(cases, X):
    """One crn_step_block call over the six f4 columns."""
    xs, AX, B, l2, reg, vals = start(cases, X, cases.cols)
    Xn, AXn, al, be, infos = X.crn_step_block(xs, B, vals, M, reg, AX=AX, l2=l2)
    return dict(xs=xs, AX=AX, B=B, l2=l2, reg=reg, vals=vals, Xn=h(Xn), AXn=h(AXn), Xn_dev=Xn, al=al, be=be,
                infos=infos)


def single(cases, c, steps, which="f4", m=M, dtype=torch.float64):
    A, cols = (cases.A, cases.cols) if which == "f4" else (cases.Ab, cases.bcols)
    b01, l2, reg = cols[c]
    loss = LogisticRegression(A, b01, l1=0, l2=l2, store_mat_vec_prod=True, dtype=dtype)
    opt = Cubic_Krylov_LS(loss=loss, reg_coef=reg, label="s", subspace_dim=m, tolerance=0, tqdm=False,
                          device_step=True)
    opt.run(x0=np.full(A.shape[1], 0.5), it_max=steps)
    return opt


def batch(cases, cols, steps, which="f4", m=M, dtype=torch.float64, **kw):
    A = cases.A if which == "f4" else cases.Ab
    loss = LogisticRegression(A, cols[0][0], l1=0, l2=0, store_mat_vec_prod=True, dtype=dtype)
    opt = Cubic_Krylov_LS_Batch(loss, len(cols), B=cases.B(cols), l2=[c[1] for c in cols],
                                reg_coef=[c[2] for c in cols], subspace_dim=m, **kw)
    opt.run(np.full(A.shape[1], 0.5), steps)
    return opt


# -------------------------------------------------------------------- pieces
@gpu
@pytest.mark.parametrize("k", [1, 3, 5, 16])
@pytest.mark.parametrize("per_column_labels", [False, True])
def test_gradient_and_value_block(cases, X, k, per_column_labels):
    rng = np.random.default_rng(k)
    xs = rng.uniform(-0.5, 0.5, (X.d, k))
    l2 = np.array([0.0 if c % 2 else 0.01 * (c + 1) for c in range(k)])
    b01 = cases.cols[0][0]
    B = np.stack([np.roll(b01, c) for c in range(k)], axis=1) if per_column_labels else b01
    xd, AX, bd = t(xs), X.matvec_block(t(xs)), t(B)
    G = h(X.gradient_block(AX, bd, xd, l2))
    vals = X.value_block(AX, bd, xd, l2)
    for c in range(k):
        bc = B[:, c] if per_column_labels else B
        assert rel_err(G[:, c], O.gradient(cases.A, bc, xs[:, c], l2[c])) < 1e-13
        want = O.value(cases.A, bc, xs[:, c], l2[c])
        assert abs(vals[c] - want) <= 1e-12 * abs(want)
        xc, bcd = t(xs[:, c]), t(bc)
        Ax = X.matvec(xc)
        assert rel_err(G[:, c], h(X.gradient(Ax, bcd, xc, l2[c]))) < 1e-13
        v1 = X.loss_mean(Ax, bcd) + (l2[c] / 2 * X.diff_norm(xc) ** 2 if l2[c] else 0.0)
        assert abs(vals[c] - v1) <= 1e-12 * abs(v1)


@gpu
def test_pieces_column_independence_is_bitwise(cases, X):
    rng = np.random.default_rng(11)
    xa, xb = rng.uniform(-0.5, 0.5, (X.d, 5)), rng.uniform(-0.5, 0.5, (X.d, 5))
    xb[:, 3], xb[:, 0] = xa[:, 1], xa[:, 4]          # two shared columns, at other positions
    l2a, l2b = np.array([0.0, 0.02, 0.0, 0.01, 0.03]), np.array([0.03, 0.0, 0.5, 0.02, 0.0])
    bd = t(cases.cols[0][0])
    out = []
    for xs, l2 in ((xa, l2a), (xb, l2b)):
        xd = t(xs)
        AX = X.matvec_block(xd)
        out.append((h(X.gradient_block(AX, bd, xd, l2)), X.value_block(AX, bd, xd, l2)))
    for ca, cb in ((1, 3), (4, 0)):
        assert same_bytes(out[0][0][:, ca], out[1][0][:, cb])
        assert out[0][1][ca] == out[1][1][cb]


@gpu
def test_pieces_fp32(cases):
    """fp32 handle against the fp64 oracle: the bound the fp32 tests give the same quantities
    (tests/test_gpu_configs.py: 1e-4 on values; gradients as its HVP bound, 1e-4)."""
    Xf = krcn.DeviceCSR(cases.A, dtype=torch.float32)
    rng = np.random.default_rng(2)
    xs = rng.uniform(-0.5, 0.5, (Xf.d, 3))
    l2 = np.array([0.0, 0.01, 0.0])
    b01 = cases.cols[0][0]
    xd, bd = t(xs, torch.float32), t(b01, torch.float32)
    AX = Xf.matvec_block(xd)
    G, vals = h(Xf.gradient_block(AX, bd, xd, l2)), Xf.value_block(AX, bd, xd, l2)
    for c in range(3):
        assert rel_err(G[:, c], O.gradient(cases.A, b01, xs[:, c], l2[c])) < 1e-4
        want = O.value(cases.A, b01, xs[:, c], l2[c])
        assert abs(vals[c] - want) <= 1e-4 * abs(want)
    Xf.close()


@gpu
def test_n_space_reduction_crosses_a_grid_stride():
    """n = 65,536 + 257 at k = 16: the n-space kernels cover 65,536 rows a grid
    stride at K = 16.  One nonzero a row with integer data; at AX = -64 (below
    logsig's -33 branch: logsig(a) = a) a loss term is (1 - b) a - a = 64 b, and
    the iterates are integers: every sum is exact, so the values are compared
    with ==.  The labels differ from column to column, also in the rows past the stride."""
    import scipy.sparse as sp
    n, d, k = 65536 + 257, 64, 16
    rows = np.arange(n)
    A = sp.csr_matrix((np.where(rows % 3 == 0, 2.0, 1.0), (rows, rows % d)), shape=(n, d))
    Xd = krcn.DeviceCSR(A)
    B = np.stack([(rows % (c + 2) == 0).astype(np.float64) for c in range(k)], axis=1)
    assert all(B[65536:, c].sum() >= 15 for c in range(k))   # rows past the stride carry weight in every column
    AX = np.full((n, k), -64.0)
    xs = np.tile(np.arange(k, dtype=np.float64), (d, 1))
    l2 = np.full(k, 2.0)
    vals = Xd.value_block(t(AX), t(B), t(xs), l2)
    for c in range(k):
        nrm = np.sqrt(float(d * c * c))
        assert vals[c] == 64.0 * B[:, c].sum() / n + 2.0 / 2.0 * (nrm * nrm)
    G = h(Xd.gradient_block(t(AX), t(B), t(xs), l2))
    R = 1.0 / (1.0 + np.exp(-AX)) - B
    assert rel_err(G, A.T @ R / n + 2.0 * xs) < 1e-13
    Xd.close()


@gpu
@pytest.mark.parametrize("transposed", [False, True])
def test_long_rows(transposed):
    """Rows over KRCN_BLOCK_LONG_ROW: in X for the guarded product of a trial, in
    X^T (the transposed matrix as the design matrix) for the gradient's pass."""
    from test_gpu_block import POS_A, long_matrix
    A = long_matrix(list(POS_A), 1)
    A = A.T.tocsr() if transposed else A
    A.sort_indices()
    n, d = A.shape
    lens = np.diff((A.T.tocsr() if transposed else A).indptr)
    assert lens.max() > _lib.KRCN_BLOCK_LONG_ROW
    Xl = krcn.DeviceCSR(A)
    rng = np.random.default_rng(4)
    xs = rng.uniform(-0.1, 0.1, (d, 3))
    b01 = (rng.random(n) < 0.5).astype(np.float64)
    l2 = np.array([0.0, 0.01, 0.0])
    xd, bd = t(xs), t(b01)
    AX = Xl.matvec_block(xd)
    G = h(Xl.gradient_block(AX, bd, xd, l2))
    vals = Xl.value_block(AX, bd, xd, l2)
    for c in range(3):
        assert rel_err(G[:, c], O.gradient(A, b01, xs[:, c], l2[c])) < 1e-13
        want = O.value(A, b01, xs[:, c], l2[c])
        assert abs(vals[c] - want) <= max(1e-12, n * 2.0 ** -53) * abs(want)   # (n = 20,011 transposed)
    Xn, AXn, _, _, infos = Xl.crn_step_block(xd, bd, vals, 5, 1e-3, AX=AX, l2=l2)
    assert all(i.solver_status in (0, 3) for i in infos)
    assert same_bytes(h(AXn), h(Xl.matvec_block(Xn)))
    Xl.close()


# ---------------------------------------------------------------- subproblem
@gpu
def test_cubic_tridiag_block_is_bitwise_the_single_call(X, f3):
    al, be, g, Ms, r0 = [], [], [], [], []
    for m in (3, 10, 50):
        for q in range(3):
            key = f"m{m}_k{q}"
            T = f3[f"{key}_T"]
            al.append(np.diag(T)), be.append(np.diag(T, 1)), g.append(float(f3[f"{key}_g"][0]))
            Ms.append(float(f3[f"{key}_M"])), r0.append(float(f3[f"{key}_r0"]))
    # m = 1 and m = 2, and an indefinite column (status 1, zeros) beside the good ones
    al += [np.array([0.7]), np.array([0.7, 0.4]), np.array([-5.0, 1.0, 1.0])]
    be += [np.array([]), np.array([0.05]), np.array([0.1, 0.1])]
    g += [0.3, 0.3, 1.0]
    Ms += [1e-3, 2.0, 1e-3]
    r0 += [0.1, 0.1, 0.1]

    def check(cols):
        s, infos = X.cubic_tridiag_block([al[c] for c in cols], [be[c] for c in cols], [g[c] for c in cols],
                                         [Ms[c] for c in cols], [r0[c] for c in cols])
        for i, c in enumerate(cols):
            s1, i1 = X.cubic_tridiag(al[c], be[c], g[c], Ms[c], r0=r0[c])
            assert same_bytes(s[i], s1), c
            for f in ("solver_it", "solver_status", "reg_coef", "lam", "model_decrease"):
                assert getattr(infos[i], f) == getattr(i1, f), (c, f)
        return s, infos

    s9, i9 = check(list(range(9)))
    assert all(i.solver_status == 0 for i in i9)
    s12, i12 = check(list(range(12)))
    assert i12[11].solver_status == 1 and not s12[11].any()
    for c in range(9):                                   # the good columns' bytes do not change
        assert same_bytes(s9[c], s12[c]) and i9[c].lam == i12[c].lam


# ------------------------------------------------------- the step, mixed batch
@gpu
def test_mixed_batch_first_step(cases, X, mixed):
    infos = mixed["infos"]
    for c in range(6):
        ref = cases.ref("f4", c, 1)[0]
        dev = single(cases, c, 1)
        i = infos[c]
        assert i.accepted == 1 and i.trials == ref["trials"] and i.solver_status == 0
        assert i.reg_coef == ref["reg_coef"] == dev.reg_coef
        assert i.solver_it == ref["its"] == dev.solver_it
        assert i.lanczos.m_eff == ref["m_eff"] == dev.last_lanczos.m_eff
        assert rel_err(mixed["Xn"][:, c], ref["x"]) < 1e-10
        assert rel_err(mixed["Xn"][:, c], h(dev.x)) < 1e-10
        assert abs(i.value_new - ref["value"]) <= 1e-10 * abs(ref["value"])
        assert abs(i.value_new - dev.value) <= 1e-10 * abs(dev.value)
        assert rel_err(mixed["al"][c], np.diag(dev.hess)) < 1e-11
        assert rel_err(mixed["be"][c], np.diag(dev.hess, 1)) < 1e-11
        want = X.diff_norm(mixed["Xn_dev"][:, c].contiguous(), mixed["xs"][:, c].contiguous())
        assert abs(i.dx_norm - want) <= 1e-13 * want
    assert infos[4].trials == 16
    assert same_bytes(mixed["AXn"], h(X.matvec_block(mixed["Xn_dev"])))


@gpu
def test_frozen_columns_do_not_see_the_backtracking_one(cases, X, mixed):
    """The fifth column runs 16 trials while the others sit frozen after trial 0:
    their columns are byte-identical to a call in which the fifth accepts at once too."""
    cols = list(cases.cols)
    cols[4] = cases.cols[0]
    xs, AX, B, l2, reg, vals = start(cases, X, cols)
    Xn, AXn, _, _, infos = X.crn_step_block(xs, B, vals, M, reg, AX=AX, l2=l2)
    assert infos[4].trials == 0
    for c in (0, 1, 2, 3, 5):
        assert same_bytes(h(Xn)[:, c], mixed["Xn"][:, c])
        assert same_bytes(h(AXn)[:, c], mixed["AXn"][:, c])
        assert infos[c].value_new == mixed["infos"][c].value_new


@gpu
def test_three_steps_through_the_driver(cases):
    opt = batch(cases, cases.cols, 3)
    assert len(opt.trace.values) == 3 and opt.its.tolist() == [3] * 6 and opt.active.all()
    xs = h(opt.xs)
    for c in range(6):
        ref = cases.ref("f4", c, 3)[-1]
        dev = single(cases, c, 3)
        assert opt.reg_coefs[c] == ref["reg_coef"] == dev.reg_coef
        assert opt.solver_its[c] == ref["solver_it"] == dev.solver_it
        assert opt.last_infos[c].lanczos.m_eff == ref["m_eff"]
        assert rel_err(xs[:, c], ref["x"]) < 1e-10
        assert rel_err(xs[:, c], h(dev.x)) < 1e-10
        assert abs(opt.values[c] - ref["value"]) <= 1e-10 * abs(ref["value"])
        assert abs(opt.values[c] - dev.value) <= 1e-10 * abs(dev.value)
        assert abs(opt.r0s[c] - dev.r0) <= 1e-10 * abs(dev.r0)


# ------------------------------------------------ the step, caps and failures
@gpu
def test_trial_cap_in_one_column(cases, X, mixed):
    xs, AX, B, l2, reg, vals = mixed["xs"], mixed["AX"], mixed["B"], mixed["l2"], mixed["reg"], mixed["vals"]
    Xn, AXn, _, _, infos = X.crn_step_block(xs, B, vals, M, reg, AX=AX, l2=l2, max_trials=2)
    assert infos[4].accepted == 0 and infos[4].trials == 2
    assert infos[4].reg_coef == 1e-9 * 0.5 / 0.5 / 0.5
    assert infos[4].value_new > vals[4] - infos[4].model_decrease
    for c in (0, 1, 2, 3, 5):
        assert infos[c].accepted == 1
        assert same_bytes(h(Xn)[:, c], mixed["Xn"][:, c]) and same_bytes(h(AXn)[:, c], mixed["AXn"][:, c])


@gpu
def test_failed_solve_in_one_column(cases, X, mixed):
    xs, AX, B, l2, reg, vals = mixed["xs"], mixed["AX"], mixed["B"], mixed["l2"], mixed["reg"], mixed["vals"]
    r0 = np.full(6, 0.1)
    r0[2] = -10.0
    Xn, AXn, _, _, infos = X.crn_step_block(xs, B, vals, M, reg, AX=AX, l2=l2, r0=r0)
    assert infos[2].solver_status == 1 and infos[2].accepted == 0 and infos[2].dx_norm == 0.0
    for c in (0, 1, 3, 4, 5):
        assert infos[c].solver_status == 0 and infos[c].trials == mixed["infos"][c].trials
        assert same_bytes(h(Xn)[:, c], mixed["Xn"][:, c]) and same_bytes(h(AXn)[:, c], mixed["AXn"][:, c])
    loss = LogisticRegression(cases.A, cases.cols[0][0], l1=0, l2=0, store_mat_vec_prod=True)
    opt = Cubic_Krylov_LS_Batch(loss, 3, reg_coef=1e-3)
    orig = loss.device_matrix.crn_step_block

    def bad_r0(*a, **kw):
        kw["r0"] = np.array([0.1, -10.0, 0.1])
        return orig(*a, **kw)

    loss.device_matrix.crn_step_block = bad_r0
    with pytest.raises(la.LinAlgError, match="column 1: .*not positive definite"):
        opt.run(cases.x0, 1)


@gpu
def test_inactive_column(cases, X, mixed):
    xs, AX, B, l2, reg, vals = mixed["xs"], mixed["AX"], mixed["B"], mixed["l2"], mixed["reg"], mixed["vals"]
    active = [1, 0, 1, 1, 1, 1]
    Xn, AXn, _, _, infos = X.crn_step_block(xs, B, vals, M, reg, AX=AX, l2=l2, active=active)
    i = infos[1]
    assert (i.accepted, i.trials, i.dx_norm) == (0, 0, 0.0) and i.value_new == vals[1] and i.reg_coef == reg[1]
    assert same_bytes(h(Xn)[:, 1], h(xs)[:, 1]) and same_bytes(h(AXn)[:, 1], h(AX)[:, 1])
    for c in (0, 2, 3, 4, 5):
        assert same_bytes(h(Xn)[:, c], mixed["Xn"][:, c]) and same_bytes(h(AXn)[:, c], mixed["AXn"][:, c])
    # AX not given, and labels that make the inactive column's residual (and so its gradient) vanish
    # up to rounding: whatever its recurrence computes (NaNs for an exact zero) reaches nothing
    B2 = B.clone()
    B2[:, 1] = 1.0 / (1.0 + torch.exp(-AX[:, 1]))
    l2z = l2.copy()
    l2z[1] = 0.0
    Xn2, AXn2, _, _, infos2 = X.crn_step_block(xs, B2, vals, M, reg, l2=l2z, active=active)
    assert same_bytes(h(Xn2)[:, 1], h(xs)[:, 1]) and same_bytes(h(AXn2)[:, 1], h(AX)[:, 1])
    assert infos2[1].value_new == vals[1] and infos2[1].trials == 0
    for c in (0, 2, 3, 4, 5):
        assert same_bytes(h(Xn2)[:, c], mixed["Xn"][:, c]) and same_bytes(h(AXn2)[:, c], mixed["AXn"][:, c])
        assert infos2[c].value_new == mixed["infos"][c].value_new


# ---------------------------------------------------------------- truncation
@gpu
@pytest.mark.parametrize("m", [10, 7])
def test_truncated_basis(cases, m):
    opt = batch(cases, cases.bcols, 1, which="brk", m=m)
    for c in range(3):
        ref = cases.ref("brk", c, 1, m)[0]
        dev = single(cases, c, 1, which="brk", m=m)
        li = opt.last_infos[c].lanczos
        assert li.m_eff == ref["m_eff"] == dev.last_lanczos.m_eff and li.breakdown == 1
        assert opt.reg_coefs[c] == dev.reg_coef == ref["reg_coef"]
        assert opt.solver_its[c] == dev.solver_it
        assert rel_err(h(opt.xs)[:, c], h(dev.x)) < 1e-10
        assert rel_err(h(opt.xs)[:, c], ref["x"]) < 1e-10


# ------------------------------------------------ other dtypes, k and refusals
@gpu
def test_fp32_two_steps(cases):
    cols = cases.cols[:3]
    opt = batch(cases, cols, 2, dtype=torch.float32)
    for c in range(3):
        dev = single(cases, c, 2, dtype=torch.float32)
        assert opt.reg_coefs[c] == dev.reg_coef and opt.solver_its[c] == dev.solver_it
        assert rel_err(h(opt.xs)[:, c], h(dev.x)) < 1e-3
        assert abs(opt.values[c] - dev.value) <= 1e-4 * abs(dev.value)


@gpu
@pytest.mark.parametrize("k", [1, 16])
def test_other_k(cases, k):
    cols = [cases.cols[c % 4] for c in range(k)]
    opt = batch(cases, cols, 1)
    for c in range(k):
        ref = cases.ref("f4", c % 4, 1)[0]
        assert opt.reg_coefs[c] == ref["reg_coef"] and opt.solver_its[c] == ref["solver_it"]
        assert rel_err(h(opt.xs)[:, c], ref["x"]) < 1e-10
        assert abs(opt.values[c] - ref["value"]) <= 1e-10 * abs(ref["value"])


@gpu
def test_tolerance_stops_one_column(cases):
    """Column 5 (reg_coef 10) takes the shortest first step: a tolerance between its
    length and the others' stops it after step 1 while the others run on."""
    first = batch(cases, cases.cols, 1)
    dx = np.array([i.dx_norm for i in first.last_infos])
    order = np.argsort(dx)
    tol = 0.5 * (dx[order[0]] + dx[order[1]])
    opt = batch(cases, cases.cols, 3, tolerance=tol)
    stopped = int(order[0])
    assert opt.its[stopped] == 1 and not opt.active[stopped]
    assert same_bytes(h(opt.xs)[:, stopped], h(first.xs)[:, stopped])
    assert all(opt.its[c] >= 2 for c in range(6) if c != stopped)


@gpu
def test_sharded_is_refused(cases):
    Xs = krcn.DeviceCSR(cases.A, shard_mode=_lib.KRCN_SHARD_ROWS)
    xs = torch.full((Xs.d, 2), 0.5, dtype=torch.float64, device=Xs.device)
    bd = torch.zeros(Xs.n, dtype=torch.float64, device=Xs.device)
    AX = torch.zeros((Xs.n, 2), dtype=torch.float64, device=Xs.device)
    for call in (lambda: Xs.crn_step_block(xs, bd, [0.7, 0.7], M, 1e-3), lambda: Xs.gradient_block(AX, bd),
                 lambda: Xs.value_block(AX, bd), lambda: Xs.cubic_tridiag_block([[1.0]], [[]], 1.0, 1.0)):
        with pytest.raises(_lib.KrcnError) as e:
            call()
        assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    Xs.close()

    class Sharded:
        shard = object()
    with pytest.raises(NotImplementedError):
        Cubic_Krylov_LS_Batch(Sharded(), 2, reg_coef=1e-3)


# ------------------------------------------------- memory and side effects
@gpu
def test_repeated_steps_allocate_nothing_and_leave_the_single_paths_alone(cases):
    Xd = krcn.DeviceCSR(cases.A)
    b01 = cases.cols[0][0]
    x, bd = t(cases.x0), t(b01)
    Ax = Xd.matvec(x)
    w = Xd.weights(Ax)
    g = Xd.gradient(Ax, bd)
    value = Xd.loss_mean(Ax, bd)

    def singles():
        y = h(Xd.hvp(w, g))
        V, al, be, _ = Xd.lanczos(w, g, M)
        xn, Axn, al2, be2, info = Xd.crn_step(x, bd, value, M, 1e-3, Ax=Ax)
        return y, h(V), al, be, h(xn), h(Axn), al2, be2, info.value_new, info.lam

    before = singles()
    xs, AX, B, l2, reg, vals = start(cases, Xd, cases.cols[:4])
    sizes = []
    for _ in range(3):
        Xd.crn_step_block(xs, B, vals, M, reg, AX=AX, l2=l2)
        sizes.append(Xd.owned_bytes())
    assert sizes[1] == sizes[2] == sizes[0]
    after = singles()
    for a, b in zip(before, after):
        assert same_bytes(np.asarray(a), np.asarray(b))
    Xd.close()
