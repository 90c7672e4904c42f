"""Krylov cubic-regularized Newton on the GPU (drop-in for optimizer/cubic.py).

Hot path (north_star): `Lanczos` + the logistic HVP run as hand-written gfx950
kernels through libkrcn; the recurrence's control state (alpha, beta, the
absolute 1e-6 breakdown test) stays on the device and only the m alphas / m-1
betas come back.  The m x m tridiagonal cubic subproblem stays on the host by
default, as in the reference, but as O(m) tridiagonal LDL^T solves (LAPACK
dpttrf/dpttrs) instead of a dense Cholesky per Newton evaluation
(cubic_solver_root_tridiag).  Cubic_Krylov_LS(device_step=True) runs the whole
step behind one library call instead (krcn_crn_step): the same subproblem in
one workgroup on the device and the line search's accept / reject test in a
device kernel, with the backtracking trials enqueued in guarded batches.

The comparison methods of cubic_newton.py run on the same device kernels:
Cubic_LS (full-space CRN: "CG" solves with device conjugate gradients on the
HVP, krcn_cg_solve — or, with device_solver=True, the whole subproblem behind
one krcn_cubic_cg call; "full" factors the dense Hessian built from HVPs) and SSCN
(coordinate subspaces: partial gradient / Hessian and the incremental Ax
update on the device).  Lanczos also accepts any callable operator.

Reference: optimizer/cubic.py — cubic_solver_root :40-75, Lanczos :77-111,
Cubic_LS :115-235, Cubic_Krylov_LS :238-319, SSCN :321-408.
"""
from __future__ import annotations

import copy
import warnings

import numpy as np
import numpy.linalg as la
import scipy.sparse as sp
import torch
from scipy.linalg import lapack, solve
from scipy.optimize import root_scalar
from scipy.sparse.linalg import spsolve

from krcn.vec import VecContext

from .loss import HessianOperator
from .optimizer import Optimizer


def cubic_solver_root(g, H, M, it_max=100, epsilon=1e-8, r0=0.1):
    """argmin_s <g,s> + 1/2 <s,Hs> + M/3 ||s||^3 on the host (cubic.py:40-75).

    Newton's method on phi(lam) = lam^2 - M^2 ||s(lam)||^2, s(lam) = -(H + lam I)^{-1} g
    (Cartis, Gould & Toint 2011, §6.1).  Returns (s, newton iterations, lam,
    model decrease).  The arithmetic is written term for term like the
    reference so the host trajectory is bit-identical given identical T."""
    g = np.asarray(g)
    m = len(g)
    if sp.issparse(H) and m >= 500:
        eye = sp.eye(m)

        def shifted_solve(lam, rhs):
            return spsolve(H + lam * eye, rhs)
    else:
        Hd = H.toarray() if sp.issparse(H) else H
        eye = np.eye(m)

        def shifted_solve(lam, rhs):
            return solve(Hd + lam * eye, rhs, assume_a="pos")

    def phi(lam):
        s_lam = -shifted_solve(lam, g)
        return lam ** 2 - M ** 2 * np.linalg.norm(s_lam) ** 2

    def dphi(lam):
        s_lam = -shifted_solve(lam, g)
        dnorm2 = -2 * np.dot(s_lam, shifted_solve(lam, s_lam))
        return 2 * lam - M ** 2 * dnorm2

    sol = root_scalar(phi, fprime=dphi, x0=r0, method="newton", maxiter=it_max, xtol=epsilon)
    lam = sol.root
    s = -shifted_solve(lam, g)
    ns = la.norm(s)
    model_decrease = lam / 2 * ns ** 2 - M / 3 * ns ** 3 - np.dot(g, s) / 2
    return s, sol.iterations, lam, model_decrease


def cubic_solver_root_tridiag(g, alphas, betas, M, it_max=100, epsilon=1e-8, r0=0.1):
    """cubic_solver_root for H = tridiag(betas, alphas, betas), the Krylov
    subspace Hessian of Cubic_Krylov_LS (cubic.py:278-285).

    Same Newton iteration on phi(lam) = lam^2 - M^2 ||s(lam)||^2 (root_scalar,
    same x0 / xtol / maxiter) and the same closing expressions as
    cubic_solver_root, but each shifted solve (T + lam I) s = rhs is a
    tridiagonal LDL^T factorisation (LAPACK dpttrf, O(m)) shared by every solve
    at the same lam, instead of a dense Cholesky (solve(assume_a='pos'),
    O(m^3)) per solve.  A shift that leaves T + lam I indefinite raises
    LinAlgError, as the dense positive-definite solve does.  Results agree with
    the dense path to rounding (tests/test_host_logic.py)."""
    g = np.asarray(g, dtype=np.float64)
    al = np.asarray(alphas, dtype=np.float64)
    be = np.asarray(betas, dtype=np.float64)
    if len(al) != len(g) or len(be) != max(len(g) - 1, 0):
        raise ValueError("alphas must have len(g) entries and betas len(g) - 1")
    fact = {}
    be_arg = be if len(be) else np.zeros(1)   # LAPACK's e has max(m - 1, 1) slots

    def shifted_solve(lam, rhs):
        f = fact.get(lam)
        if f is None:
            dd, ee, info = lapack.dpttrf(al + lam, be_arg)
            if info != 0:
                raise la.LinAlgError("T + lam I is not positive definite")
            fact.clear()
            fact[lam] = f = (dd, ee)
        x, info = lapack.dpttrs(f[0], f[1], rhs)
        if info != 0:
            raise la.LinAlgError(f"dpttrs failed (info {info})")
        return x

    def phi(lam):
        s_lam = -shifted_solve(lam, g)
        return lam ** 2 - M ** 2 * np.linalg.norm(s_lam) ** 2

    def dphi(lam):
        s_lam = -shifted_solve(lam, g)
        dnorm2 = -2 * np.dot(s_lam, shifted_solve(lam, s_lam))
        return 2 * lam - M ** 2 * dnorm2

    sol = root_scalar(phi, fprime=dphi, x0=r0, method="newton", maxiter=it_max, xtol=epsilon)
    lam = sol.root
    s = -shifted_solve(lam, g)
    ns = la.norm(s)
    model_decrease = lam / 2 * ns ** 2 - M / 3 * ns ** 3 - np.dot(g, s) / 2
    return s, sol.iterations, lam, model_decrease


def _lanczos_callable(A, v, m, tol):
    """cubic.py:77-111 over a plain callable A, every vector operation on the
    device (krcn_vctx kernels): A is called once per step.  A numpy v means a
    numpy operator (called with host vectors, results uploaded) and returns V
    as a numpy (d, m_eff) array; a device tensor v keeps A's traffic on the
    device and returns a (d, m_eff) device view."""
    numpy_mode = not isinstance(v, torch.Tensor)
    if numpy_mode:
        if not torch.cuda.is_available():
            raise RuntimeError("Lanczos runs on the GPU (no CPU path exists)")
        dev = torch.device("cuda", torch.cuda.current_device())
        vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    else:
        vd = v.detach().contiguous()
        dev = vd.device
    ctx = VecContext.for_device(dev)
    d = vd.numel()

    def apply(q):
        y = A(q.cpu().numpy() if numpy_mode else q)
        if isinstance(y, torch.Tensor):
            return y.to(device=dev, dtype=vd.dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(y).ravel(), dtype=np.float64)).to(dev, vd.dtype)

    V = torch.zeros((m, d), dtype=vd.dtype, device=dev)     # cubic.py:88 (zeros: the quirk column)
    ctx.div(vd, np.sqrt(ctx.dot(vd, vd)), out=V[0])          # cubic.py:85-89
    alphas = np.zeros(m)
    betas = np.zeros(max(m - 1, 0))
    beta = 0.0
    v_pre = None
    vj = V[0]
    z = torch.empty_like(vd)
    j = 0
    for j in range(m - 1):                                   # cubic.py:92-103
        y = apply(vj)
        alpha, beta = ctx.lz_step(y, vj, v_pre, beta, z)
        alphas[j] = alpha
        if np.abs(beta) < tol:
            break
        betas[j] = beta
        v_pre = vj
        ctx.div(z, beta, out=V[j + 1])
        vj = V[j + 1]
    m_eff = m
    if m > 1 and j < m - 2:                                  # cubic.py:105-108
        m_eff = j + 1
        alphas = alphas[:j + 1]
        betas = betas[:j]
    alphas[-1] = ctx.dot(vj, apply(vj))                       # cubic.py:109
    Vt = V[:m_eff].T
    return (Vt.cpu().numpy() if numpy_mode else Vt), alphas, betas, beta


def Lanczos(A, v, m=10, reorth=False, tol=1e-6, V=None):
    """m-step three-term Lanczos (cubic.py:77-111), on the GPU.

    A: the device Hessian operator of a LogisticRegression
    (`loss.hess_operator(x)`: the fused device recurrence, krcn_lanczos), or any
    callable v -> A v, such as the reference's `lambda v: loss.hess_vec_prod(x,
    v)` (cubic.py:273): it is called once per step and the recurrence's vector
    work runs on the device (krcn_lz_ext_step).  v: the start vector (numpy or
    device tensor).  Returns (V, alphas, betas, beta) like the reference: V is
    (d, m_eff) — a device view for the operator / a device v, a numpy array for
    a numpy v with a callable —, alphas / betas numpy arrays after the
    reference's truncation rule, beta the last computed norm.
    reorth=True adds CGS2 full reorthogonalisation (not in the reference; fused
    operator only)."""
    if not isinstance(A, HessianOperator):
        if not callable(A):
            raise TypeError("Lanczos needs a callable operator or loss.hess_operator(x)")
        if reorth:
            raise NotImplementedError("reorth=True needs the fused device operator loss.hess_operator(x)")
        if V is not None:
            raise ValueError("V is only accepted with the fused device operator")
        return _lanczos_callable(A, v, int(m), tol)
    X = A.X
    g = A.loss.to_device(v)
    Vb, alphas, betas, info = X.lanczos(A.w, g, m, reorth=reorth, tol=tol, l2=A.l2, V=V)
    return Vb[:info.m_eff].T, alphas, betas, info.beta_last


class Cubic_Krylov_LS(Optimizer):
    """Krylov cubic regularized Newton with line search (cubic.py:238-319).

    reg_coef: cubic regularization estimate (required: the Lipschitz estimate
    of the reference's default is outside the hot path); subspace_dim: Krylov
    dimension m; solver_eps: tolerance of the host subproblem; beta:
    backtracking factor.  Build-only extras: reorth (CGS2 in Lanczos), tol
    (absolute breakdown threshold, 1e-6 as cubic.py:98), device_step (one
    krcn_crn_step call per step: the subproblem and the line search's decision
    run on the device; unsharded losses and the tridiagonal subproblem only).
    With device_step the loss's f_opt / x_opt follow the iterate each step
    keeps, not the rejected trials (their vectors are overwritten on the
    device), and the stopping test reads the step length the call reports."""

    def __init__(self, reg_coef=None, subspace_dim=100, solver_eps=1e-8, beta=0.5, *args,
                 reorth=False, breakdown_tol=1e-6, dense_subproblem=False, device_step=False, **kwargs):
        super().__init__(*args, **kwargs)
        if device_step and dense_subproblem:
            raise ValueError("device_step=True solves the tridiagonal subproblem: dense_subproblem must be False")
        if device_step and getattr(self.loss, "shard", None) is not None:
            raise NotImplementedError("device_step=True is implemented for unsharded problems")
        self.device_step = bool(device_step)
        self._dx_norm = None
        self.solver_it = 0
        self.subspace_dim = subspace_dim
        self.solver_eps = solver_eps
        self.beta = beta
        self.r0 = 0.1
        self.value = None
        self.reorth = reorth
        self.breakdown_tol = breakdown_tol
        self.dense_subproblem = dense_subproblem
        self.reg_coef = self.loss.hessian_lipschitz if reg_coef is None else reg_coef
        self._V = None
        self.last_lanczos = None

    def _basis(self):
        X = self.loss.device_matrix
        m = self.subspace_dim
        if self._V is None or self._V.shape != (m, X.d):
            self._V = torch.empty((m, X.d), dtype=X.dtype, device=X.device)
        return self._V

    def step(self):
        """One Krylov-CRN step (cubic.py:265-309): grad -> Lanczos -> host cubic
        subproblem over T -> x + V s -> backtracking (at most 20 trials)."""
        if self.device_step:
            return self._step_on_device()
        loss = self.loss
        X = loss.device_matrix
        if self.value is None:
            self.value = loss.value(self.x)
        grad = loss.gradient(self.x)
        op = loss.hess_operator(self.x)
        V, alphas, betas, info = X.lanczos(op.w, grad, self.subspace_dim, reorth=self.reorth,
                                           tol=self.breakdown_tol, l2=op.l2, V=self._basis())
        self.last_lanczos = info
        self.hess = np.diag(alphas) + np.diag(betas, -1) + np.diag(betas, 1)
        e1 = np.zeros(len(alphas))
        e1[0] = 1
        self.grad = info.gnorm * e1
        reg_coef = self.reg_coef * self.beta
        s_new, solver_it, r0_new, model_decrease = self._subproblem(alphas, betas, reg_coef)
        x_new = X.basis_combine(V, s_new, self.x)
        value_new = loss.value(x_new)
        trials = 0
        while value_new > self.value - model_decrease and trials < 20:
            reg_coef = reg_coef / self.beta
            s_new, solver_it, r0_new, model_decrease = self._subproblem(alphas, betas, reg_coef)
            x_new = X.basis_combine(V, s_new, self.x)
            value_new = loss.value(x_new)
            trials += 1
        self.x = x_new
        self.reg_coef = reg_coef
        self.value = value_new
        self.r0 = r0_new
        self.solver_it += solver_it

    def _step_on_device(self):
        """The same step as one krcn_crn_step call; the state afterwards is the
        host path's (x, reg_coef, value, r0, solver_it, last_lanczos, hess,
        grad) and the loss's cache holds X x_new for the new iterate."""
        loss = self.loss
        X = loss.device_matrix
        if self.value is None:
            self.value = loss.value(self.x)
        x_new, Ax_new, alphas, betas, info = X.crn_step(
            self.x, loss._b_dev, self.value, self.subspace_dim, self.reg_coef, Ax=loss._device_Ax(self.x),
            V=self._basis(), reorth=self.reorth, tol=self.breakdown_tol, l2=float(loss.l2), ls_beta=self.beta,
            r0=self.r0, solver_eps=self.solver_eps, max_trials=20)
        self.last_lanczos = info.lanczos
        self.hess = np.diag(alphas) + np.diag(betas, -1) + np.diag(betas, 1)
        e1 = np.zeros(len(alphas))
        e1[0] = 1
        self.grad = info.lanczos.gnorm * e1
        if info.solver_status == 1:
            raise la.LinAlgError("T + lam I is not positive definite")
        if info.solver_status == 2:
            raise ArithmeticError("cubic subproblem: the derivative of phi was zero")
        loss.adopt_product(x_new, Ax_new)
        loss.note_value(x_new, info.value_new)
        self.x = x_new
        self.reg_coef = info.reg_coef
        self.value = info.value_new
        self.r0 = info.lam
        self.solver_it += info.solver_it
        self._dx_norm = info.dx_norm

    def _keep_previous_iterate(self):
        if not self.device_step:
            super()._keep_previous_iterate()

    def _step_length(self):
        return self._dx_norm if self.device_step else super()._step_length()

    def _subproblem(self, alphas, betas, reg_coef):
        """The m x m cubic subproblem over T = tridiag(betas, alphas, betas)
        (cubic.py:285-286): O(m) tridiagonal solves, or the reference's dense
        solver with dense_subproblem=True."""
        if self.dense_subproblem:
            return cubic_solver_root(self.grad, self.hess, reg_coef, epsilon=self.solver_eps, r0=self.r0)
        return cubic_solver_root_tridiag(self.grad, alphas, betas, reg_coef, epsilon=self.solver_eps,
                                         r0=self.r0)

    def init_run(self, *args, **kwargs):
        super().init_run(*args, **kwargs)
        self.trace.solver_its = [0]
        self.loss.reset()
        self._dx_norm = None

    def update_trace(self):
        super().update_trace()
        self.trace.solver_its.append(self.solver_it)


class _BatchTrace:
    """What Cubic_Krylov_LS_Batch.run records: one length-k array of loss values per step."""

    def __init__(self):
        self.values = []


class Cubic_Krylov_LS_Batch:
    """k Krylov-CRN problems over one design matrix, advanced together: one
    krcn_crn_step_block call per step, column c being one step of
    `Cubic_Krylov_LS(device_step=True)` on problem c (cubic.py:265-309) with the
    line search decided per column on the device.

    loss: an unsharded LogisticRegression (its matrix, dtype, default labels and
    l2).  k: the number of problems.  B: None (every column uses the loss's
    labels) or an (n, k) block of labels (one-vs-rest).  l2 (default: the
    loss's) and reg_coef: a float or a length-k sequence.  subspace_dim,
    solver_eps, beta, breakdown_tol as Cubic_Krylov_LS; tolerance > 0 makes a
    column whose step length falls below it inactive (its iterate is kept).

    After run(): xs (device (d, k)), values, reg_coefs, r0s, solver_its
    (cumulative), its (steps each column took), trials (backtracking trials,
    cumulative), active, and trace.values."""

    def __init__(self, loss, k, B=None, l2=None, reg_coef=None, subspace_dim=10, solver_eps=1e-8, beta=0.5,
                 breakdown_tol=1e-6, tolerance=0):
        from krcn import _lib
        from .loss import _labels01
        if getattr(loss, "shard", None) is not None:
            raise NotImplementedError("Cubic_Krylov_LS_Batch is implemented for unsharded problems")
        k = int(k)
        if not 1 <= k <= _lib.KRCN_BLOCK_MAX:
            raise ValueError(f"k must lie in [1, {_lib.KRCN_BLOCK_MAX}], got {k}")
        if reg_coef is None:
            raise ValueError("reg_coef is required (a float or one per column)")
        self.loss = loss
        self.k = k
        X = loss.device_matrix
        if B is None:
            self._b = loss._b_dev
        else:
            Bh = np.asarray(B)
            if Bh.shape != (X.n, k):
                raise ValueError(f"B must be an ({X.n}, {k}) block of labels, got shape {Bh.shape}")
            Bh = np.stack([_labels01(Bh[:, c]) for c in range(k)], axis=1)
            self._b = torch.from_numpy(np.ascontiguousarray(Bh, dtype=loss._np_dtype())).to(loss.device)
        self.l2s = X._per_column(float(loss.l2) if l2 is None else l2, k, "l2")
        self.reg_coefs = X._per_column(reg_coef, k, "reg_coef").copy()
        self.subspace_dim = int(subspace_dim)
        self.solver_eps = solver_eps
        self.beta = beta
        self.breakdown_tol = breakdown_tol
        self.tolerance = tolerance
        self.trace = _BatchTrace()
        self.xs = None
        self.values = None
        self.last_infos = None
        self._V = None

    def _block(self, x0):
        loss, k = self.loss, self.k
        x0 = x0.detach().cpu().numpy() if isinstance(x0, torch.Tensor) else np.asarray(x0)
        d = loss.device_matrix.d
        if x0.shape == (d,):
            x0 = np.repeat(x0[:, None], k, axis=1)
        elif x0.shape != (d, k):
            raise ValueError(f"x0 must have shape ({d},) or ({d}, {k}), got {x0.shape}")
        return torch.from_numpy(np.ascontiguousarray(x0, dtype=loss._np_dtype())).to(loss.device)

    def run(self, x0, it_max):
        """At most it_max steps from x0 ((d,): every column starts there, or
        (d, k)); ends early when no column is active.  Returns the trace."""
        X, k, m = self.loss.device_matrix, self.k, self.subspace_dim
        self.xs = self._block(x0)
        AX = X.matvec_block(self.xs)
        self.values = X.value_block(AX, self._b, self.xs, self.l2s).copy()
        self.r0s = np.full(k, 0.1)
        self.solver_its = np.zeros(k, dtype=np.int64)
        self.its = np.zeros(k, dtype=np.int64)
        self.trials = np.zeros(k, dtype=np.int64)
        self.active = np.ones(k, dtype=bool)
        self.trace = _BatchTrace()
        if self._V is None or tuple(self._V.shape) != (m, X.d, k):
            self._V = torch.empty((m, X.d, k), dtype=X.dtype, device=X.device)
        spare = (torch.empty_like(self.xs), torch.empty_like(AX))
        for _ in range(int(it_max)):
            if not self.active.any():
                break
            X_new, AX_new, _, _, infos = X.crn_step_block(
                self.xs, self._b, self.values, m, self.reg_coefs, AX=AX, V=self._V, active=self.active,
                tol=self.breakdown_tol, l2=self.l2s, ls_beta=self.beta, r0=self.r0s, solver_eps=self.solver_eps,
                max_trials=20, X_new=spare[0], AX_new=spare[1])
            self.last_infos = infos
            for c in range(k):
                if not self.active[c]:
                    continue
                if infos[c].solver_status == 1:
                    raise la.LinAlgError(f"column {c}: T + lam I is not positive definite")
                if infos[c].solver_status == 2:
                    raise ArithmeticError(f"column {c}: cubic subproblem: the derivative of phi was zero")
            spare, self.xs, AX = (self.xs, AX), X_new, AX_new
            for c in range(k):
                if not self.active[c]:
                    continue
                info = infos[c]
                self.values[c] = info.value_new
                self.reg_coefs[c] = info.reg_coef
                self.r0s[c] = info.lam
                self.solver_its[c] += info.solver_it
                self.its[c] += 1
                self.trials[c] += info.trials
                if self.tolerance > 0 and info.dx_norm < self.tolerance:
                    self.active[c] = False
            self.trace.values.append(self.values.copy())
        return self.trace


class Cubic_LS(Optimizer):
    """Full-space cubic regularized Newton with line search (cubic.py:115-235;
    Nesterov & Polyak 2006), on the device kernels.

    cubic_solver="CG": every linear solve of the subproblem's Newton iteration
    is device conjugate gradients on v -> hess_vec_prod(x, v) + lam v
    (krcn_cg_solve, scipy cg's loop and stopping rule with rtol = solver_eps,
    the reference's `cg(..., tol=epsilon)`, cubic.py:152-182).
    cubic_solver="full": the dense Hessian (loss.hessian, built from HVPs on the
    device) goes to the host subproblem solver, cubic.py:184-188.
    Arguments and trace as the reference.

    device_solver=True (not in the reference; off by default, "CG" only,
    unsharded losses) solves the subproblem behind one krcn_cubic_cg call
    instead of a host root_scalar loop over krcn_cg_solve: the Newton iteration
    on lam and every CG solve's control stay on the device.  The line search
    stays on the host.  A failed solve raises: LinAlgError (H + lam I not
    positive definite), ArithmeticError (phi' = 0), FloatingPointError (a
    non-finite lam, rho or p.q).

    gram_hessian=True (not in the reference; off by default, "full" only) builds
    the dense Hessian of every step as one Gram product on the device
    (loss.hessian(x, gram=True)); the loss needs a dense X^T image."""

    def __init__(self, reg_coef=None, cubic_solver="CG", solver_it_max=100, solver_eps=1e-8,
                 beta=0.5, *args, device_solver=False, gram_hessian=False, **kwargs):
        super().__init__(*args, **kwargs)
        if gram_hessian and cubic_solver != "full":
            raise ValueError('gram_hessian=True builds the dense Hessian of the "full" subproblem solver; '
                             f"got cubic_solver={cubic_solver!r}")
        self.gram_hessian = bool(gram_hessian)
        if device_solver:
            if cubic_solver != "CG":
                raise ValueError('device_solver=True runs the "CG" subproblem solver on the device; '
                                 f"got cubic_solver={cubic_solver!r}")
            if getattr(self.loss, "shard", None) is not None:
                raise NotImplementedError("device_solver=True is implemented for unsharded problems")
        self.device_solver = bool(device_solver)
        self.solver_it = 0
        self.solver_it_max = solver_it_max
        self.solver_eps = solver_eps
        self.beta = beta
        self.r0 = 0.1
        self.residuals = []
        self.value = None
        self.cg_iterations = 0          # device CG iterations (not in the reference's trace)
        self.cg_unconverged = 0         # CG solves that hit maxiter (scipy's info > 0)
        self.reg_coef = self.loss.hessian_lipschitz if reg_coef is None else reg_coef
        if cubic_solver == "CG":
            self.cubic_solver = self.cubic_solver_root_CG
        elif cubic_solver == "full":
            self.cubic_solver = self.cubic_solver_root_full
        else:
            print("Error: cubic_solver not recognized")

    def cubic_solver_root_CG(self, M, it_max=100, epsilon=1e-8, r0=0.1):
        """cubic_solver_root with every (H + lam I)^{-1} applied by device CG
        (cubic.py:152-182).  CG is linear in its right-hand side and IEEE
        negation is exact, so solving with g and negating reproduces the
        reference's cg(H_lambda, -g) without materialising -g.  Returns
        (s, newton iterations, lam, model decrease); s is a device d-vector."""
        loss = self.loss
        X = loss.device_matrix
        g = self.grad
        w = loss._weights_for(self.x)
        l2 = float(loss.l2)
        sol_cache = {}
        # a relative residual below ~10 ulp of the working precision is out of
        # reach: asked for 1e-8 in fp32, every solve would run its 10 d
        # iterations without ever stopping (fp64 keeps the reference's tol)
        rtol = max(float(epsilon), 10.0 * float(torch.finfo(X.dtype).eps))
        if self.device_solver:
            return self._cubic_solver_on_device(M, it_max, epsilon, r0, w, rtol)

        def cg(lam, rhs):
            x, info = X.cg_solve(w, rhs, shift=l2 + lam, rtol=rtol)
            self.cg_iterations += info.iterations
            if not info.converged:
                self.cg_unconverged += 1
                if self.cg_unconverged == 1:
                    warnings.warn(f"device CG stopped at maxiter = {info.iterations} with ||r|| = "
                                  f"{info.residual_norm:.3e} (rtol {rtol:.1e}); counted in cg_unconverged")
            return x

        def neg_s(lam):          # -s(lam) = (H + lam I)^{-1} g
            y = sol_cache.get(lam)
            if y is None:
                sol_cache.clear()
                sol_cache[lam] = y = cg(lam, g)
            return y

        def func(lam):
            return lam ** 2 - M ** 2 * X.diff_norm(neg_s(lam)) ** 2

        def grad(lam):
            y = neg_s(lam)                   # s = -y; H_lam^{-1} s = -H_lam^{-1} y
            phi_lam_grad = -2 * X.dot(y, cg(lam, y))
            return 2 * lam - M ** 2 * phi_lam_grad

        sol = root_scalar(func, fprime=grad, x0=r0, method="newton", maxiter=it_max, xtol=epsilon)
        r = sol.root
        y = cg(r, g)
        norm_s = X.diff_norm(y)
        model_decrease = r / 2 * norm_s ** 2 - M / 3 * norm_s ** 3 + X.dot(g, y) / 2
        s = VecContext.for_device(X.device).axpy(-1.0, y, torch.zeros_like(y))
        return s, sol.iterations, r, model_decrease

    def _cubic_solver_on_device(self, M, it_max, epsilon, r0, w, rtol):
        """cubic_solver_root_CG behind one krcn_cubic_cg call; same return values."""
        X = self.loss.device_matrix
        s, info = X.cubic_cg(w, self.grad, M, l2=float(self.loss.l2), r0=r0, eps=epsilon, it_max=it_max,
                             cg_rtol=rtol)
        self.cg_iterations += info.cg_iterations
        if info.cg_unconverged:
            if self.cg_unconverged == 0:
                warnings.warn(f"device CG stopped at maxiter in {info.cg_unconverged} of {info.cg_solves} solves "
                              f"(rtol {rtol:.1e}); counted in cg_unconverged")
            self.cg_unconverged += info.cg_unconverged
        if info.solver_status == 1:
            raise la.LinAlgError("H + lam I is not positive definite (conjugate gradients met p.q <= 0)")
        if info.solver_status == 2:
            raise ArithmeticError("cubic subproblem: the derivative of phi was zero")
        if info.solver_status == 4:
            raise FloatingPointError("cubic subproblem: a non-finite lam, rho or p.q ended the solve")
        return s, info.solver_it, info.lam, info.model_decrease

    def cubic_solver_root_full(self, M, it_max=100, epsilon=1e-8, r0=0.1):
        """The host subproblem over the dense Hessian (cubic.py:184-188)."""
        g = self.loss.to_host(self.grad)
        return cubic_solver_root(g, self.hess, M, it_max=it_max, epsilon=epsilon, r0=r0)

    def _add(self, s):
        s = self.loss.to_device(s)
        return VecContext.for_device(self.loss.device).axpy(1.0, s, self.x)

    def step(self):
        """cubic.py:190-224: gradient, (dense Hessian), cubic subproblem,
        x + s, backtracking on reg_coef until sufficient decrease."""
        loss = self.loss
        if self.value is None:
            self.value = loss.value(self.x)
        self.grad = loss.gradient(self.x)
        if self.cubic_solver == self.cubic_solver_root_full:
            self.hess = loss.hessian(self.x, gram=True) if self.gram_hessian else loss.hessian(self.x)
        if loss.norm(self.grad) < self.tolerance:
            return
        reg_coef = self.reg_coef * self.beta
        s_new, solver_it, r0_new, model_decrease = self.cubic_solver(
            reg_coef, self.solver_it_max, self.solver_eps, r0=self.r0)
        x_new = self._add(s_new)
        value_new = loss.value(x_new)
        while value_new > self.value - model_decrease:
            reg_coef = reg_coef / self.beta
            s_new, solver_it, r0_new, model_decrease = self.cubic_solver(
                reg_coef, self.solver_it_max, self.solver_eps, r0=self.r0)
            x_new = self._add(s_new)
            value_new = loss.value(x_new)
        self.x = x_new
        self.reg_coef = reg_coef
        self.value = value_new
        self.r0 = r0_new
        self.solver_it += solver_it

    def init_run(self, *args, **kwargs):
        super().init_run(*args, **kwargs)
        self.trace.solver_its = [0]
        self.loss.reset()

    def update_trace(self):
        super().update_trace()
        self.trace.solver_its.append(self.solver_it)


class SSCN(Optimizer):
    """Stochastic subspace cubic Newton, coordinate version (cubic.py:321-408;
    Hanzely et al. 2020, §7.1), on the device kernels: the coordinate gradient
    and Hessian (loss.partial_gradient / partial_hessian), the coordinate
    update of x and the incremental Ax update (loss.update_mat_vec_product)
    run on the GPU; the m x m subproblem on the host, as in the reference.

    device_step=True (not in the reference; off by default) runs the whole step
    behind one krcn_sscn_step call instead: the gradient and the Hessian block
    stay on the device, the dense subproblem is solved there in one workgroup
    and the line search's decision is taken by a device kernel, with the trials
    enqueued in guarded batches (unsharded losses, subspace_dim <=
    KRCN_SSCN_MAX = 128, at most 20 backtracking trials).  The rng draw is the
    host path's.  Differences: self.grad and self.hess are not brought back
    (the step does not set them), and the loss's f_opt / x_opt follow the iterate each step
    keeps, not the rejected trials, whose vectors are overwritten on the
    device.  The host loop backtracks without a cap; the device step stops
    after 20 rejected trials and keeps the last one, as Cubic_Krylov_LS does:
    that step warns (RuntimeWarning) and is counted in `capped_steps`.
    `last_trials` holds the backtracking trials of the last step on both
    paths.

    subproblem="tridiag" (device_step=True only; default "cholesky") runs the
    device step through krcn_sscn_step_tridiag: the block is reduced once per
    step to tridiagonal form and every trial solves the tridiagonal subproblem,
    which lifts the cap on subspace_dim to KRCN_SSCN_TRIDIAG_MAX = 1024.  The
    differences of the device step above carry over unchanged."""

    def __init__(self, reg_coef=None, subspace_dim=100, solver_eps=1e-8, beta=0.5, *args, device_step=False,
                 subproblem="cholesky", **kwargs):
        super().__init__(*args, **kwargs)
        if subproblem not in ("cholesky", "tridiag"):
            raise ValueError(f'subproblem must be "cholesky" or "tridiag", got {subproblem!r}')
        if subproblem == "tridiag" and not device_step:
            raise ValueError('subproblem="tridiag" is the device step\'s: it needs device_step=True')
        if device_step:
            from krcn import _lib
            if getattr(self.loss, "shard", None) is not None:
                raise NotImplementedError("device_step=True is implemented for unsharded problems")
            if subproblem == "tridiag":
                if not 1 <= int(subspace_dim) <= _lib.KRCN_SSCN_TRIDIAG_MAX:
                    raise ValueError(f'device_step=True with subproblem="tridiag" needs 1 <= subspace_dim <= '
                                     f"{_lib.KRCN_SSCN_TRIDIAG_MAX}, got {subspace_dim}")
            elif not 1 <= int(subspace_dim) <= _lib.KRCN_SSCN_MAX:
                raise ValueError(f"device_step=True needs 1 <= subspace_dim <= {_lib.KRCN_SSCN_MAX}, "
                                 f"got {subspace_dim}")
        self.device_step = bool(device_step)
        self.subproblem = subproblem
        self.last_trials = 0
        self.capped_steps = 0       # device steps that ended at the trial cap without an accepted trial
        self.reg_coef = reg_coef
        self.solver_it = 0
        self.subspace_dim = subspace_dim
        self.solver_eps = solver_eps
        self.beta = beta
        self.r0 = 0.1
        self.residuals = []
        self.value = None
        self.tolerance = 0
        if reg_coef is None:
            self.reg_coef = self.loss.hessian_lipschitz
        self.reuse = False

    def _coordinate_step(self, I_dev, s_sub):
        x_new = self.x.clone()
        x_new[I_dev] = self.x[I_dev] + torch.from_numpy(np.asarray(s_sub, dtype=np.float64)).to(
            self.x.device, self.x.dtype)
        return x_new

    def step(self):
        """cubic.py:349-399."""
        if self.device_step:
            return self._step_on_device()
        loss = self.loss
        if self.value is None:
            self.value = loss.value(self.x)
        I = self.rng.choice(self.dim, size=self.subspace_dim, replace=False)
        I_dev = torch.from_numpy(np.asarray(I, dtype=np.int64)).to(self.x.device)
        self.grad = loss.partial_gradient(self.x, I)
        self.hess = loss.partial_hessian(self.x, I)
        reg_coef = max(self.reg_coef * self.beta, np.finfo(float).eps)
        Ax = copy.deepcopy(loss._mat_vec_prod)
        s_new_sub, solver_it, r0_new, model_decrease = cubic_solver_root(
            self.grad, self.hess, reg_coef, r0=self.r0, epsilon=np.finfo(float).eps)
        x_new = self._coordinate_step(I_dev, s_new_sub)
        loss.update_mat_vec_product(Ax, s_new_sub, I)
        value_new = loss.value(x_new)
        trials = 0
        while value_new > self.value - model_decrease:
            reg_coef = reg_coef / self.beta
            s_new_sub, solver_it, r0_new, model_decrease = cubic_solver_root(
                self.grad, self.hess, reg_coef, r0=self.r0, epsilon=np.finfo(float).eps)
            x_new = self._coordinate_step(I_dev, s_new_sub)
            loss.update_mat_vec_product(Ax, s_new_sub, I)
            value_new = loss.value(x_new)
            trials += 1
        self.last_trials = trials
        self.x = x_new
        self.reg_coef = reg_coef
        self.value = value_new
        self.r0 = r0_new
        self.solver_it += solver_it

    def _step_on_device(self):
        """The same step as one krcn_sscn_step call: the state afterwards is
        the host path's x, reg_coef, value, r0 and solver_it, and the loss's
        cache holds X x_new for the new iterate."""
        loss = self.loss
        X = loss.device_matrix
        if self.value is None:
            self.value = loss.value(self.x)
        I = self.rng.choice(self.dim, size=self.subspace_dim, replace=False)
        x_new, Ax_new, info = X.sscn_step(
            I, self.x, loss._b_dev, self.value, self.reg_coef, Ax=loss._device_Ax(self.x), l2=float(loss.l2),
            ls_beta=self.beta, r0=self.r0, solver_eps=np.finfo(float).eps, max_trials=20,
            subproblem=self.subproblem)
        if info.solver_status == 1:
            raise la.LinAlgError("H + lam I is not positive definite")
        if info.solver_status == 2:
            raise ArithmeticError("cubic subproblem: the derivative of phi was zero")
        if not info.accepted:
            self.capped_steps += 1
            warnings.warn(f"SSCN device step: no trial met the decrease test within {info.trials} backtracking "
                          f"trials (reg_coef {info.reg_coef:.3e}); the last trial is kept", RuntimeWarning)
        loss.adopt_product(x_new, Ax_new)
        loss.note_value(x_new, info.value_new)
        self.x = x_new
        self.reg_coef = info.reg_coef
        self.value = info.value_new
        self.r0 = info.lam
        self.solver_it += info.solver_it
        self.last_trials = info.trials

    def init_run(self, *args, **kwargs):
        super().init_run(*args, **kwargs)
        self.trace.solver_its = [0]
        self.loss.reset()

    def update_trace(self):
        super().update_trace()
        self.trace.solver_its.append(self.solver_it)
