"""Logistic-regression oracle on the GPU (drop-in for optimizer/loss.py).

Same constructor and methods as the reference's `LogisticRegression`
(loss.py:179-302): value, gradient, hess_vec_prod, mat_vec_product, reset, n,
dim, f_opt, x_opt.  The design matrix lives in HBM behind a libkrcn handle
(krcn.DeviceCSR); every product with X or X^T is a hand-written gfx950 kernel.

Vectors: methods accept numpy arrays (returning numpy, as the reference does)
or torch tensors on the handle's device (returning device tensors — the
Krylov-CRN step keeps everything on the GPU this way).

Caching (loss.py:266-277, store_mat_vec_prod=True): Ax and the Hessian weights
s(1-s) are kept for the last x.  A device x hits the cache when it is the same
tensor object at the same version (the cache holds a reference, so its memory
cannot be recycled under it); a numpy x hits when it is array_equal to the
last numpy x, the reference's own test (loss.py:361-375).  The weights are
recomputed only when Ax changes — the reference recomputes them on every HVP
(loss.py:296-297) with identical results.

The comparison methods' pieces (dense `hessian`, the SSCN `partial_*` methods,
`update_mat_vec_product`) and the smoothness estimates run on the device
kernels for unsharded problems (they raise NotImplementedError on a shard);
l1 / prox regularizers are out of scope and raise
NotImplementedError.
"""
from __future__ import annotations

import copy
import warnings

import numpy as np
import torch

import krcn
from krcn import _lib
from krcn.labels import labels01 as _labels01


class _PinnedArena:
    """Pinned host storage for trace checkpoints, allocated in chunks of
    several d-vectors (about 64 MB each) so a checkpoint is one async copy
    rather than a pinned allocation plus a synchronous one."""

    _CHUNK_BYTES = 64 << 20

    def __init__(self):
        self.chunk = None
        self.used = 0

    def take(self, numel, dtype):
        c = self.chunk
        if c is None or self.used == c.shape[0] or c.shape[1] != numel or c.dtype != dtype:
            per = max(1, self._CHUNK_BYTES // max(1, numel * torch.empty((), dtype=dtype).element_size()))
            self.chunk = torch.empty((per, numel), dtype=dtype, pin_memory=True)
            self.used = 0
        row = self.chunk[self.used]
        self.used += 1
        return row


class Oracle:
    """Base objective (loss.py:29-113): l1/l2 coefficients and best-value tracking."""

    def __init__(self, l1=0, l2=0, l2_in_prox=False, regularizer=None, seed=42):
        if l1 < 0.0:
            raise ValueError(f"Invalid value for l1 regularization: {l1}")
        if l2 < 0.0:
            raise ValueError(f"Invalid value for l2 regularization: {l2}")
        if l2 == 0.0 and l2_in_prox:
            warnings.warn("The value of l2 is set to 0, so l2_in_prox is changed to False.")
            l2_in_prox = False
        self.l1 = l1
        self.l2 = 0 if l2_in_prox else l2
        self.l2_in_prox = l2_in_prox
        self.x_opt = None
        self.f_opt = np.inf
        self.regularizer = regularizer
        self.seed = seed
        if (l1 > 0 or l2_in_prox) or regularizer is not None:
            raise NotImplementedError(
                "l1 / prox regularizers are outside the device hot path (SURVEY.md §2)")
        self.rng = np.random.default_rng(seed)

    def set_seed(self, seed):
        self.seed = seed
        self.rng = np.random.default_rng(seed)

    def value(self, x):
        """Objective value with best-iterate tracking (loss.py:66-73)."""
        val = self._value(x)
        if val < self.f_opt:
            self.x_opt = x.clone() if isinstance(x, torch.Tensor) else copy.deepcopy(x)
            self.f_opt = val
        return val


class HessianOperator:
    """v -> hess_vec_prod(x, v) at a fixed x, on the device.

    The reference builds `lambda v: loss.hess_vec_prod(self.x, v)`
    (cubic.py:273) and hands it to Lanczos; passing this object instead lets
    `optimizer.cubic.Lanczos` run the fused device recurrence."""

    def __init__(self, loss, x):
        self.loss = loss
        self.x = x
        self.X = loss.device_matrix
        self.w = loss._weights_for(x)
        self.l2 = float(loss.l2)

    def __call__(self, v):
        return self.loss.hess_vec_prod(self.x, v)


class LogisticRegression(Oracle):
    """Logistic loss f(x) = mean((1-b) Ax - logsig(Ax)) (+ l2/2 ||x||^2) on the GPU.

    A: scipy sparse (converted to CSR) or dense n x d matrix; b: binary labels.
    device / dtype: where and in which precision the device copy of A lives
    (fp64 by default, as the reference computes).  shard: optional
    krcn.dist.ShardSpec for multi-GPU runs (krcn.dist.shard_problem builds it).
    format: None keeps the handle's format policy, "auto" names that policy
    explicitly (KRCN_FORMAT_AUTO), "dense" stores A and A^T as row-major images
    without indices (nearly dense A such as gisette, madelon or duke; unsharded
    only), an int is a KRCN_FORMAT_* value.
    values: "f32" stores the plans' matrix values in fp32 (each rounded;
    vectors, sums and the recurrence keep the dtype: the objective is then that
    of double(float(A))) and "f32-exact" does so only if no value of A changes
    by it; None or "full" keeps the dtype.  Dense, window and jagged plans
    honour it, so it needs a format named by the caller that can take such a
    plan: "dense", "auto", KRCN_FORMAT_WINDOW or KRCN_FORMAT_JAG (under "auto" a
    plan with a wave or sorted pass stays full width: plan_value_bytes()).
    format=None, wave and sorted raise ValueError.
    """

    def __init__(self, A, b, store_mat_vec_prod=False, *args, device=None, dtype=torch.float64,
                 shard=None, lanes=(0, 0), format=None, values=None, **kwargs):
        super().__init__(*args, **kwargs)
        if format is None or (isinstance(format, (int, np.integer)) and not isinstance(format, bool)):
            fmt = None if format is None else int(format)
        elif format == "dense":
            fmt = _lib.KRCN_FORMAT_DENSE
        elif format == "auto":
            fmt = _lib.KRCN_FORMAT_AUTO
        else:
            raise ValueError(f"format must be None, 'auto', 'dense' or a KRCN_FORMAT_* int, got {format!r}")
        if values not in (None, "full", "f32", "f32-exact"):
            raise ValueError(f"values must be None, 'full', 'f32' or 'f32-exact', got {values!r}")
        narrowing = (_lib.KRCN_FORMAT_AUTO, _lib.KRCN_FORMAT_WINDOW, _lib.KRCN_FORMAT_JAG, _lib.KRCN_FORMAT_DENSE)
        if values not in (None, "full") and fmt not in narrowing:
            raise ValueError(f"values={values!r} needs format='dense', 'auto', KRCN_FORMAT_WINDOW or KRCN_FORMAT_JAG: "
                             "only dense, window and jagged passes store narrowed values")
        import scipy.sparse as sp
        self.A = A
        self.b = _labels01(b)
        self.store_mat_vec_prod = store_mat_vec_prod
        self.reuse = False
        self.shard = shard
        A_local = sp.csr_matrix(A) if shard is None else shard.A_local
        b_local = np.asarray(self.b, dtype=np.float64) if shard is None else shard.b_local(self.b)
        self.n, self.dim = A.shape
        mode = _lib.KRCN_SHARD_NONE if shard is None else shard.mode
        self.device_matrix = krcn.DeviceCSR(A_local, device=device, dtype=dtype,
                                            n_global=self.n, shard_mode=mode, lanes=lanes)
        if fmt is not None:
            self.device_matrix.set_format(fmt)
        if values not in (None, "full"):
            self.device_matrix.set_value_storage(values)
        if shard is not None and shard.comm is not None:
            self.device_matrix.attach_comm(shard.comm)
        if fmt == _lib.KRCN_FORMAT_DENSE:
            # the images are built here, not inside the first compute call
            self.device_matrix.plan_info()
        self.device = self.device_matrix.device
        self.dtype = dtype
        self._b_dev = torch.from_numpy(b_local.astype(self._np_dtype())).to(self.device)
        self.x_last = 0.0
        self._mat_vec_prod = None
        self._cache_x = None        # device tensor whose Ax is cached
        self._cache_ver = None
        self._cache_np = None       # numpy copy for array_equal hits
        self._w = None

    # ------------------------------------------------------------ vectors
    def _np_dtype(self):
        return np.float64 if self.dtype == torch.float64 else np.float32

    def _local_d(self, x):
        """Slice a global d-vector to this rank's columns (COLS shards)."""
        if self.shard is not None and x.shape[0] == self.dim and self.device_matrix.d != self.dim:
            return x[self.shard.col_lo:self.shard.col_hi]
        return x

    def to_device(self, x, copy=False):
        """Device d-vector (local block of it in a column-sharded run)."""
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.device, dtype=self.dtype)
            t = self._local_d(t)
            return t.clone().contiguous() if copy else t.contiguous()
        x = np.asarray(x)
        if sp_issparse(x):
            x = x.toarray().ravel()
        x = self._local_d(np.ascontiguousarray(x, dtype=self._np_dtype()))
        return torch.from_numpy(np.ascontiguousarray(x)).to(self.device)

    def to_host(self, x):
        return x.detach().to("cpu").numpy().copy() if isinstance(x, torch.Tensor) else np.array(x)

    def to_host_async(self, x):
        """A checkpoint copy of x that does not wait for the device: an async
        D2H copy on the current stream into pinned host memory, returned as a
        numpy view of it.  The view holds x's value once the stream has passed
        the copy — every later Lanczos call synchronises the stream, and
        `sync()` does so explicitly (Optimizer.run calls it before returning)."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            return self.to_host(x)
        if not hasattr(self, "_arena"):
            self._arena = _PinnedArena()
        row = self._arena.take(x.numel(), x.dtype)
        row.copy_(x.detach().reshape(-1), non_blocking=True)
        return row.numpy()

    def sync(self):
        """Wait for the async checkpoint copies on this loss's device."""
        if getattr(self, "_arena", None) is not None and self._arena.used:
            torch.cuda.current_stream(self.device).synchronize()

    # ------------------------------------------------ stored iterates
    _DEV_ITER_CAP = 8 << 30   # device bytes of kept iterate copies, at most

    def keep_device_iterate(self, x):
        """A device copy of a trace iterate (Optimizer.update_trace), or None
        past the budget (min(8 GiB, a quarter of the device)); the copy's bytes
        return to the budget when the trace drops it.  The budget counts the
        GLOBAL d-vector, so every rank of a sharded run (whose local d differ
        in a column split) keeps copies of the same iterates and
        values_of_iterates issues the same collectives on all of them."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            return None
        nbytes = int(self.dim) * x.element_size()
        if not hasattr(self, "_dev_iter_bytes"):
            self._dev_iter_bytes = [0]
            # (hipMemGetInfo; torch.cuda.get_device_properties re-counts the
            # devices through amdsmi until torch has initialised, which failed
            # as "Invalid device id" with 8 virtual-rank threads asking at once)
            total = torch.cuda.mem_get_info(self.device)[1]
            self._dev_iter_cap = min(self._DEV_ITER_CAP, total // 4)
        if self._dev_iter_bytes[0] + nbytes > self._dev_iter_cap:
            return None
        c = x.detach().clone()
        import weakref
        self._dev_iter_bytes[0] += nbytes
        weakref.finalize(c, _release, self._dev_iter_bytes, nbytes)
        return c

    def values_of_iterates(self, xs, dev):
        """[self.value(x) for x in xs] (opt_trace.py:39-41) with the iterates
        that have device copies in `dev` (id(x) -> (x, copy)) evaluated by one
        krcn_loss_values submission; the rest, and the best-iterate tracking
        (loss.py:66-73: f_opt / x_opt updated in order), as the loop does."""
        idx = [i for i, x in enumerate(xs) if id(x) in dev and dev[id(x)][0] is x]
        vals = [None] * len(xs)
        if idx:
            cop = [dev[id(xs[i])][1] for i in idx]
            for i, v, c in zip(idx, self.device_matrix.loss_values(cop, self._b_dev), cop):
                vals[i] = v + self.l2 / 2 * self.norm_diff(c) ** 2 if self.l2 != 0 else v
        out = []
        for i, x in enumerate(xs):
            if vals[i] is None:
                out.append(self.value(x))
                continue
            v = vals[i]
            if v < self.f_opt:
                self.x_opt = x.clone() if isinstance(x, torch.Tensor) else copy.deepcopy(x)
                self.f_opt = v
            out.append(v)
        return out

    def copy_vector(self, x):
        return x.clone() if isinstance(x, torch.Tensor) else copy.deepcopy(x)

    def norm_diff(self, a, b=None):
        """||a - b||_2 on the device (optimizer.py:110; all ranks in a sharded run)."""
        a = self.to_device(a)
        b = None if b is None else self.to_device(b)
        return self.device_matrix.diff_norm(a, b, space=_lib.KRCN_SPACE_D)

    def norm(self, x):
        return self.norm_diff(x)

    def any_rank(self, flag):
        """Rank-wide OR of a host flag (keeps SPMD loops in lockstep)."""
        if self.shard is None or self.shard.comm is None or self.shard.world == 1:
            return bool(flag)
        return self.shard.comm.any(flag)

    # ------------------------------------------------------- Ax / weights
    def reset(self):
        """loss.py:283-286."""
        self.reuse = False
        self.x_last = 0.0
        self._mat_vec_prod = None
        self._cache_x = self._cache_np = None
        self._w = None

    def _cached(self, x):
        if not self.store_mat_vec_prod or self._mat_vec_prod is None:
            return False
        if self.reuse:            # SSCN keeps Ax current itself (loss.py:267, :279-281)
            return True
        if isinstance(x, torch.Tensor):
            return x is self._cache_x and x._version == self._cache_ver
        return self._cache_np is not None and np.array_equal(np.asarray(x), self._cache_np)

    def _device_Ax(self, x):
        if self._cached(x):
            return self._mat_vec_prod
        xd = self.to_device(x)
        Ax = self.device_matrix.matvec(xd)
        if self.store_mat_vec_prod:
            self._mat_vec_prod = Ax
            self._w = None
            if isinstance(x, torch.Tensor):
                self._cache_x, self._cache_ver, self._cache_np = x, x._version, None
            else:
                self._cache_x, self._cache_ver = None, None
                self._cache_np = np.array(x, copy=True)
            self.x_last = x
        return Ax

    def adopt_product(self, x, Ax):
        """Make Ax the cached product of the device iterate x (a step that
        formed X x itself hands it over, so the next gradient runs no matvec)."""
        if not self.store_mat_vec_prod:
            return
        self._mat_vec_prod = Ax
        self._w = None
        self._cache_x, self._cache_ver, self._cache_np = x, x._version, None
        self.x_last = x

    def note_value(self, x, val):
        """Best-iterate tracking (loss.py:66-73) for a value computed elsewhere."""
        if val < self.f_opt:
            self.x_opt = x.clone()
            self.f_opt = val

    def _weights_for(self, x):
        Ax = self._device_Ax(x)
        if self.store_mat_vec_prod and Ax is self._mat_vec_prod:
            if self._w is None:
                self._w = self.device_matrix.weights(Ax)
            return self._w
        return self.device_matrix.weights(Ax)

    def mat_vec_product(self, x):
        """Ax (loss.py:266-277); numpy in -> numpy out."""
        Ax = self._device_Ax(x)
        return Ax if isinstance(x, torch.Tensor) else self.to_host(Ax)

    # --------------------------------------------------------- oracle calls
    def _value(self, x):
        """mean((1-b) Ax - logsig(Ax)) + l2/2 ||x||^2 (loss.py:215-220)."""
        Ax = self._device_Ax(x)
        val = self.device_matrix.loss_mean(Ax, self._b_dev)
        if self.l2 != 0:
            val = val + self.l2 / 2 * self.norm_diff(x) ** 2
        return val

    def gradient(self, x):
        """X^T (expit(Ax) - b) / n (+ l2 x) (loss.py:223-232)."""
        Ax = self._device_Ax(x)
        xd = self.to_device(x) if self.l2 != 0 else None
        g = self.device_matrix.gradient(Ax, self._b_dev, xd, float(self.l2))
        return g if isinstance(x, torch.Tensor) else self.to_host(g)

    def hess_vec_prod(self, x, v, grad_dif=False, eps=None):
        """X^T (w * X v) / n + l2 v with w = s(1-s), s = expit(Ax) (loss.py:289-302)."""
        if grad_dif:
            gx = self.gradient(x)
            return (self.gradient(x + eps * v) - gx) / eps
        w = self._weights_for(x)
        y = self.device_matrix.hvp(w, self.to_device(v), l2=float(self.l2))
        return y if isinstance(v, torch.Tensor) else self.to_host(y)

    def hess_mat_prod(self, x, V):
        """H(x) V for a (d, k') block V of any k' >= 1: the block HVP
        (krcn_hvp_block) over blocks of at most KRCN_BLOCK_MAX columns, two
        passes over the matrix per block instead of two per column, with the
        weights hoisted once.  numpy in -> numpy out, torch in -> device tensor."""
        self._no_shards("hess_mat_prod")
        is_torch = isinstance(V, torch.Tensor)
        if V.ndim != 2 or V.shape[0] != self.dim or V.shape[1] < 1:
            raise ValueError(f"V must be a ({self.dim}, k) block with k >= 1, got shape {tuple(V.shape)}")
        w = self._weights_for(x)
        X = self.device_matrix
        Vd = V.to(device=self.device, dtype=self.dtype) if is_torch else \
            torch.from_numpy(np.ascontiguousarray(V, dtype=self._np_dtype())).to(self.device)
        out = torch.empty((self.dim, Vd.shape[1]), dtype=self.dtype, device=self.device)
        for c0 in range(0, Vd.shape[1], _lib.KRCN_BLOCK_MAX):
            c1 = min(c0 + _lib.KRCN_BLOCK_MAX, Vd.shape[1])
            out[:, c0:c1] = X.hvp_block(w, Vd[:, c0:c1].contiguous(), l2=float(self.l2))
        return out if is_torch else self.to_host(out)

    def lanczos_block(self, xs, G, m, l2=None):
        """k Lanczos recurrences (cubic.py:77-111) over this matrix in lockstep
        (krcn_lanczos_block), column c started from G[:, c].  xs of shape (d,):
        one iterate, its weights shared by every column; xs of shape (d, k): k
        iterates, column c on the Hessian at xs[:, c] (one block product X xs,
        then the block weights).  l2: a float or one per column (default: this
        loss's l2 for every column).  Returns (V, alphas, betas, infos) as
        DeviceCSR.lanczos_block; numpy G -> numpy V of shape (m, d, k)."""
        self._no_shards("lanczos_block")
        is_torch = isinstance(G, torch.Tensor)
        if G.ndim != 2 or G.shape[0] != self.dim or not 1 <= G.shape[1] <= _lib.KRCN_BLOCK_MAX:
            raise ValueError(f"G must be a ({self.dim}, k) block with 1 <= k <= {_lib.KRCN_BLOCK_MAX}, "
                             f"got shape {tuple(G.shape)}")
        k = int(G.shape[1])
        X = self.device_matrix

        def block(a):
            if isinstance(a, torch.Tensor):
                return a.to(device=self.device, dtype=self.dtype).contiguous()
            return torch.from_numpy(np.ascontiguousarray(a, dtype=self._np_dtype())).to(self.device)

        if xs.ndim == 1:
            w = self._weights_for(xs)
        elif xs.ndim == 2 and tuple(xs.shape) == (self.dim, k):
            w = X.weights_block(X.matvec_block(block(xs)))
        else:
            raise ValueError(f"xs must have shape ({self.dim},) or ({self.dim}, {k}), got {tuple(xs.shape)}")
        V, alphas, betas, infos = X.lanczos_block(w, block(G), m, l2=float(self.l2) if l2 is None else l2)
        return (V if is_torch else self.to_host(V)), alphas, betas, infos

    def hess_operator(self, x):
        return HessianOperator(self, x)

    # ------------------------------------- full-space CRN and SSCN pieces
    def _unit_columns(self, x, cols):
        """Columns `cols` of the Hessian at x as device tensors: H e_c by the
        device HVP (e_c one unit vector each; the l2 term lands on the diagonal)."""
        self._no_shards("the dense / coordinate Hessian")
        w = self._weights_for(x)
        X = self.device_matrix
        e = torch.zeros(self.dim, dtype=self.dtype, device=self.device)
        out = []
        for c in cols:
            e[int(c)] = 1.0
            out.append(X.hvp(w, e, l2=float(self.l2)))
            e[int(c)] = 0.0
        return out

    def _no_shards(self, what):
        if self.shard is not None:
            raise NotImplementedError(f"{what} is implemented for unsharded problems")

    def hessian(self, x, block=None, gram=False):
        """Dense Hessian X^T diag(w) X / n + l2 I (loss.py:249-255): the
        coordinate-block kernel over all columns for d <= KRCN_COORD_MAX, one
        device HVP per column above that; numpy (d, d), for the full-space CRN
        at small d.  block=k (1..KRCN_BLOCK_MAX) builds the d > KRCN_COORD_MAX
        Hessian from block HVPs over k unit vectors at a time instead: d / k
        matrix reads, not d (the sums of a long row then run in the block
        kernels' order, so entries may differ from block=None in the last bits).
        gram=True (any d; needs a dense X^T image: format="dense", or
        device_matrix.set_pass_format(2, KRCN_FORMAT_DENSE)) builds it as one
        weighted Gram product in fp64 on the matrix instruction
        (DeviceCSR.hessian_gram): exactly symmetric, entries within rounding of
        the default's; the library's error is raised when pass 2 is not dense."""
        if gram and block is not None:
            raise ValueError("gram=True builds the Hessian in one product: it takes no block")
        self._no_shards("the dense / coordinate Hessian")
        if gram:
            H = self.device_matrix.hessian_gram(self._weights_for(x), l2=float(self.l2))
            return H.cpu().numpy()
        if block is not None and not 1 <= int(block) <= _lib.KRCN_BLOCK_MAX:
            raise ValueError(f"block must be None or 1..{_lib.KRCN_BLOCK_MAX}, got {block!r}")
        if self.dim <= _lib.KRCN_COORD_MAX:
            return self.device_matrix.coord_hessian(np.arange(self.dim), self._device_Ax(x), float(self.l2))
        if block is not None:
            return self._hessian_by_blocks(x, int(block))
        cols = self._unit_columns(x, range(self.dim))
        return torch.stack(cols, dim=1).cpu().numpy().astype(np.float64)

    def _hessian_by_blocks(self, x, k):
        w = self._weights_for(x)
        X = self.device_matrix
        H = torch.empty((self.dim, self.dim), dtype=self.dtype, device=self.device)
        E = torch.zeros((self.dim, k), dtype=self.dtype, device=self.device)
        for c0 in range(0, self.dim, k):
            kc = min(k, self.dim - c0)
            Ec = E if kc == k else torch.zeros((self.dim, kc), dtype=self.dtype, device=self.device)
            diag = torch.arange(kc, device=self.device)
            Ec[c0 + diag, diag] = 1.0
            H[:, c0:c0 + kc] = X.hvp_block(w, Ec, l2=float(self.l2))
            Ec[c0 + diag, diag] = 0.0
        return H.cpu().numpy().astype(np.float64)

    def partial_gradient(self, x, I):
        """Coordinates I of the gradient (loss.py:234-247) by the coordinate
        kernel, which reads the columns I of X alone; numpy (len(I),)."""
        self._no_shards("partial_gradient")
        Ax = self._device_Ax(x)
        xd = self.to_device(x) if self.l2 != 0 else None
        return self.device_matrix.coord_gradient(I, Ax, self._b_dev, xd, float(self.l2))

    def partial_hessian(self, x, I):
        """The I x I block of the Hessian (loss.py:257-264) by the coordinate
        kernel; a scipy sparse (CSR) matrix like the reference's
        A_weighted @ A[:, I] / n + l2 eye."""
        import scipy.sparse as sp
        self._no_shards("partial_hessian")
        return sp.csr_matrix(self.device_matrix.coord_hessian(I, self._device_Ax(x), float(self.l2)))

    def update_mat_vec_product(self, Ax, delta, I):
        """Ax + A[:, I] delta becomes the cached product, reused for every x
        until reset() (loss.py:279-281, SSCN's incremental update), by the
        coordinate kernel in scipy's csc_matvec order."""
        self._no_shards("update_mat_vec_product")
        # the reference starts the cache as zeros(n) (loss.py:283-286): with
        # store_mat_vec_prod=False SSCN hands back that never-written zero
        # vector (here: None) and the sum is never read (mat_vec_product
        # recomputes A x), so A[:, I] delta alone stands in for it
        self._mat_vec_prod = self.device_matrix.coord_update(I, delta, Ax)
        self._w = None
        self.reuse = True

    # ------------------------------------------------- smoothness constants
    def _lambda_max_gram(self, m=64):
        """Largest eigenvalue of X^T X / n: the top Ritz value of a device
        Lanczos (CGS2-reorthogonalised) on v -> X^T (1 * X v) / n from a
        constant start vector, the eigenvalue svds(A, k=1)^2 / n refers to."""
        X = self.device_matrix
        ones_n = torch.ones(X.n, dtype=self.dtype, device=self.device)
        # the basis is m x d: at most 512 vectors and 1 GiB of them
        esz = torch.empty((), dtype=self.dtype).element_size()
        cap = max(1, min(512, self.dim, (1 << 30) // max(1, X.d * esz)))

        def top_ritz(v0, m):
            # the top Ritz pair of an m-step Lanczos, grown until its true
            # residual ||H y - theta y|| is below 1e-8 theta (a Ritz value is
            # only a lower bound on lambda_max until it has converged)
            while True:
                V, al, be, info = X.lanczos(ones_n, v0, m, reorth=True, tol=1e-14)
                T = np.diag(al) + np.diag(be, -1) + np.diag(be, 1)
                th, S = np.linalg.eigh(T)
                theta = float(th[-1])
                if info.breakdown or m >= cap:   # an invariant subspace: theta is exact in it
                    return theta, bool(info.breakdown)
                zero = torch.zeros(X.d, dtype=self.dtype, device=self.device)
                y = X.basis_combine(V, S[:, -1], zero)
                Hy = X.hvp(ones_n, y)
                res = X.diff_norm(Hy, (theta * y).contiguous())
                if res <= 1e-8 * abs(theta):
                    return theta, False
                m = min(2 * m, cap)

        m = max(1, min(int(m), self.dim))
        theta, invariant = top_ritz(torch.ones(X.d, dtype=self.dtype, device=self.device), m)
        if invariant and self.dim > 1:
            # the constant start spans an invariant subspace that may miss the
            # top eigenvector (mixed-sign features): restart at random, keep the max
            g = torch.Generator(device="cpu").manual_seed(self.seed)
            v1 = torch.randn(X.d, generator=g, dtype=torch.float64).to(self.device, self.dtype)
            theta = max(theta, top_ritz(v1, m)[0])
        return theta

    @property
    def smoothness(self):
        """L of the logistic loss (loss.py:308-320): 0.25 sigma_max(A)^2 / n + l2,
        or the Frobenius bound for n, d > 20000.  sigma_max^2 / n comes from the
        device Lanczos (the reference calls ARPACK's svds); ||A||_F^2 from a
        device dot of the values."""
        if getattr(self, "_smoothness", None) is not None:
            return self._smoothness
        self._no_shards("smoothness")
        X = self.device_matrix
        if self.dim > 20000 and self.n > 20000:
            warnings.warn("The matrix is too large to estimate the smoothness constant, so Frobenius "
                          "estimate is used instead.")
            from krcn.vec import VecContext
            fro2 = VecContext.for_device(self.device).dot(X.data, X.data)
            self._smoothness = 0.25 * fro2 / self.n + self.l2
        else:
            self._smoothness = 0.25 * self._lambda_max_gram() + self.l2
        return self._smoothness

    @property
    def hessian_lipschitz(self):
        """Lipschitz estimate of the Hessian, max ||a_i|| * max |third derivative|
        * ||A||^2 = (4 (L - l2)) max ||a_i|| / (6 sqrt 3) (loss.py:339-347)."""
        if getattr(self, "_hessian_lipschitz", None) is not None:
            return self._hessian_lipschitz
        import scipy.sparse as sp
        A = sp.csr_matrix(self.A)
        lens = np.diff(A.indptr)
        sq = np.add.reduceat(A.data ** 2, A.indptr[:-1][lens > 0]) if A.nnz else np.zeros(1)
        a_max = float(np.sqrt(sq.max()))
        A_norm = (self.smoothness - self.l2) * 4
        self._hessian_lipschitz = A_norm * a_max / (6 * np.sqrt(3))
        return self._hessian_lipschitz

    @staticmethod
    def inner_prod(x, y):
        return x @ y

    @staticmethod
    def outer_prod(x, y):
        return np.outer(x, y)

    @staticmethod
    def is_equal(x, y):
        """loss.py:361-375 for dense inputs."""
        if x is None:
            return y is None
        if y is None:
            return False
        return np.array_equal(x, y)


def _release(counter, nbytes):
    counter[0] -= nbytes


def sp_issparse(x):
    import scipy.sparse as sp
    return sp.issparse(x)
