"""Device-resident sparse design matrix: the Python face of a krcn_csr handle.

`DeviceCSR` uploads a scipy CSR matrix (the reference's LogisticRegression.A,
optimizer/loss.py:188) to HBM as torch tensors, asks libkrcn to build the
explicit, row-order-stable transpose (the reference multiplies by the zero-copy
CSC view A.T, loss.py:227,302), and exposes every C-ABI entry point as a method
taking torch device tensors.  All launches go to torch's current stream.
"""
from __future__ import annotations

import ctypes

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._lib import call

_DTYPES = {torch.float64: _lib.KRCN_F64, torch.float32: _lib.KRCN_F32}


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class DeviceCSR:
    """X (n x d) in CSR on one GPU, plus X^T in CSR, behind libkrcn.

    shard_mode / n_global describe how this block relates to the global matrix
    (include/krcn.h, KRCN_SHARD_*).  Vectors passed to the methods have the
    block's local lengths: n-vectors of length `n`, d-vectors of length `d`.
    """

    def __init__(self, A, device=None, dtype=torch.float64, n_global=None,
                 shard_mode=_lib.KRCN_SHARD_NONE, lanes=(0, 0), slicing=0, fmt=0, pass_formats=None,
                 values=0):
        if not torch.cuda.is_available():
            raise RuntimeError("krcn.DeviceCSR needs a HIP device (no CPU fallback exists)")
        if dtype not in _DTYPES:
            raise TypeError(f"dtype must be torch.float64 or torch.float32, got {dtype}")
        A = sp.csr_matrix(A)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.dtype = dtype
        self.n, self.d = (int(s) for s in A.shape)
        self.nnz = int(A.nnz)
        self.n_global = int(n_global) if n_global is not None else self.n
        self.shard_mode = shard_mode
        self.indptr = torch.from_numpy(np.ascontiguousarray(A.indptr, dtype=np.int32)).to(self.device)
        self.indices = torch.from_numpy(np.ascontiguousarray(A.indices, dtype=np.int32)).to(self.device)
        np_dt = np.float64 if dtype == torch.float64 else np.float32
        self.data = torch.from_numpy(np.ascontiguousarray(A.data, dtype=np_dt)).to(self.device)
        self._h = ctypes.c_void_p()
        self._comm = None
        self._fn_lanczos = _lib.load().krcn_lanczos
        self._lz_bufs = None
        self._reorth_m = 0       # CGS2 workspace reserved for Lanczos m <= this
        _lib.load()
        # the uploads above ran on the current stream; the library builds on its own
        torch.cuda.current_stream(self.device).synchronize()
        call("krcn_csr_create", self.device.index, self.n, self.d, self.nnz, _ptr(self.indptr),
             _ptr(self.indices), _ptr(self.data), _DTYPES[dtype], self.n_global, shard_mode,
             ctypes.byref(self._h))
        self.set_lanes(*lanes)
        self.set_slicing(slicing)
        self.set_format(fmt)
        if pass_formats is not None:
            for k, f in enumerate(pass_formats):
                self.set_pass_format(k + 1, f)
        self.set_value_storage(values)

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().krcn_csr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def owned_bytes(self) -> int:
        b = ctypes.c_int64()
        call("krcn_csr_owned_bytes", self._h, ctypes.byref(b))
        return int(b.value)

    def set_lanes(self, lanes_x=0, lanes_xt=0):
        """Row-group width for X / X^T kernels: 0 auto, 1 sequential (scipy order), 2..64."""
        call("krcn_csr_set_lanes", self._h, int(lanes_x), int(lanes_xt))
        self._replan()

    def set_slicing(self, slicing=0):
        """0 auto, 1 off, or a forced slice count (multiple of 8) for both passes."""
        call("krcn_csr_set_slicing", self._h, int(slicing))
        self._replan()

    def set_format(self, fmt=0):
        """Tile format: 0 auto, 1 wave tiles (CSR order), 2 sorted block tiles, 3 LDS windows, 4 jagged,
        5 dense (row-major images of X and X^T, no indices; never picked by auto)."""
        call("krcn_csr_set_format", self._h, int(fmt))
        self._replan()

    def set_pass_format(self, pass_, fmt):
        """Tile format of one pass (1: X, 2: X^T), overriding set_format for it; -1 restores it."""
        call("krcn_csr_set_pass_format", self._h, int(pass_), int(fmt))
        self._replan()

    _VALUES = {"full": _lib.KRCN_VALUES_FULL, "f32": _lib.KRCN_VALUES_F32, "f32-exact": _lib.KRCN_VALUES_F32_EXACT}

    def set_value_storage(self, values=0):
        """Stored width of the plans' matrix values: "full" / 0 the handle's dtype, "f32" / 1 fp32 (each
        value rounded; arithmetic, vectors and sums keep the dtype), "f32-exact" / 2 fp32 only if no
        value of the matrix changes by it.  Dense, window and jagged passes honour it (a window or
        jagged pass only when the other pass narrows too, so both passes see one matrix); wave and
        sorted passes keep full width.  plan_value_bytes() reports what each pass stores."""
        if isinstance(values, str):
            if values not in self._VALUES:
                raise ValueError(f'values must be "full", "f32" or "f32-exact", got {values!r}')
            values = self._VALUES[values]
        call("krcn_csr_set_value_storage", self._h, int(values))
        self._replan()

    def plan_value_bytes(self):
        """{'pass1': bytes, 'pass2': bytes} per stored matrix value of each pass's plan."""
        buf = (ctypes.c_int * 2)()
        call("krcn_csr_plan_value_bytes", self._h, buf)
        return {"pass1": int(buf[0]), "pass2": int(buf[1])}

    def _multi_rank(self):
        return self._comm is not None and getattr(self._comm, "world", 1) > 1

    def _replan(self):
        # a handle of a multi-rank communicator builds plans only in explicit
        # calls, never inside a compute call its peers wait on (include/krcn.h)
        if self._multi_rank():
            self.reserve(1)

    def reserve(self, m_max, reorth=False):
        """Build the pass plans and reserve krcn_lanczos's workspace for m <= m_max
        (krcn_csr_reserve): later lanczos calls up to m_max allocate nothing."""
        call("krcn_csr_reserve", self._h, int(m_max), int(bool(reorth)))
        if reorth:
            self._reorth_m = max(self._reorth_m, int(m_max))

    def set_graph(self, on=True):
        """hipGraph replay of repeated lanczos() calls (krcn_csr_set_graph; off by default)."""
        call("krcn_csr_set_graph", self._h, int(bool(on)))

    def set_placement_trials(self, trials=-1):
        """Placement probe at plan builds (krcn_csr_set_placement_trials): -1 auto, 0 off, 1..8."""
        call("krcn_csr_set_placement_trials", self._h, int(trials))
        self._replan()

    def set_placement_keep(self, keep=-1):
        """Which probed placement is kept (krcn_csr_set_placement_keep): -1 the fastest, 0..7 placement
        min(keep, probed - 1) whatever the timings say, at plan builds and after the Lanczos-call search."""
        call("krcn_csr_set_placement_keep", self._h, int(keep))
        self._replan()

    def placement_info(self):
        """The placement probe of the last plan build ({'probed', 'kept', 'hot_mb', 'policy', 'keep', 'us':
        [per placement, probe HVP]}) and the search over the first Lanczos calls ({'lanczos': {'timed',
        'kept', 'm', 'stage', 'ms': [per placement, one call each]}}; stage 0: not started, s >= 1: the next
        eligible call times placement s - 1, -1: finished)."""
        buf = (ctypes.c_double * 24)()
        call("krcn_csr_placement_info", self._h, buf)
        keep = ctypes.c_int(-1)   # (the 24 doubles are all taken: the override has a getter of its own)
        call("krcn_csr_get_placement_keep", self._h, ctypes.byref(keep))
        k, kl = int(buf[0]), int(buf[12])
        return {"probed": k, "kept": int(buf[1]), "hot_mb": round(buf[2], 1), "policy": int(buf[3]),
                "keep": int(keep.value),
                "us": [round(buf[4 + i], 2) for i in range(k)],
                "lanczos": {"timed": kl, "kept": int(buf[13]), "m": int(buf[14]), "stage": int(buf[15]),
                            "ms": [round(buf[16 + i], 4) for i in range(kl)]}}

    def plan_info(self):
        """{'pass1': (slices, lanes, tiles, grid), 'pass2': (...)}; slices < 0 marks sorted tiles,
        a dense pass reports its row groups as tiles."""
        buf = (ctypes.c_int * 8)()
        call("krcn_csr_plan_info", self._h, buf)
        return {"pass1": tuple(buf[0:4]), "pass2": tuple(buf[4:8])}

    _FORMAT_NAMES = {1: "wave", 2: "sorted", 3: "window-slices", 4: "window-accum", 5: "jagged", 6: "dense"}

    def plan_format(self):
        """{'pass1': name, 'pass2': name}: wave, sorted, window-slices, window-accum, jagged or dense."""
        buf = (ctypes.c_int * 2)()
        call("krcn_csr_plan_format", self._h, buf)
        return {"pass1": self._FORMAT_NAMES[buf[0]], "pass2": self._FORMAT_NAMES[buf[1]]}

    _STEP_NAMES = ("generic", "fused-window", "fused-sorted", "fused-small", "fused-small-xt", "two-launch",
                   "early", "early-cols", "early-rows")

    def lanczos_step(self, reorth=False):
        """The step a lanczos(.., reorth=reorth) call would run on the handle as it stands
        (krcn_csr_lanczos_step): generic, fused-window, fused-sorted, fused-small, fused-small-xt,
        two-launch, early, early-cols or early-rows.  Not collective."""
        step = ctypes.c_int(-1)
        call("krcn_csr_lanczos_step", self._h, int(bool(reorth)), ctypes.byref(step))
        return self._STEP_NAMES[step.value]

    def attach_comm(self, comm):
        call("krcn_csr_attach_comm", self._h, comm.handle if comm is not None else None)
        self._comm = comm

    def transpose_arrays(self):
        """(colptr, rowidx, vals) of the device-built X^T, as device tensors."""
        colptr = torch.empty(self.d + 1, dtype=torch.int32, device=self.device)
        rowidx = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
        vals = torch.empty(self.nnz, dtype=self.dtype, device=self.device)
        call("krcn_csr_get_transpose", self._h, _ptr(colptr), _ptr(rowidx), _ptr(vals),
             _stream(self.device))
        return colptr, rowidx, vals

    # -- helpers -----------------------------------------------------------
    def _check(self, t, length, name):
        if t is None:
            raise ValueError(f"{name} is required")
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise TypeError(f"{name} must be a torch tensor on {self.device}")
        if t.dtype != self.dtype:
            raise TypeError(f"{name} must have dtype {self.dtype}, got {t.dtype}")
        if not t.is_contiguous() or t.dim() != 1 or t.numel() != length:
            raise ValueError(f"{name} must be a contiguous 1-D tensor of length {length}, "
                             f"got shape {tuple(t.shape)}")
        return t

    def empty_n(self):
        return torch.empty(self.n, dtype=self.dtype, device=self.device)

    def empty_d(self):
        return torch.empty(self.d, dtype=self.dtype, device=self.device)

    # -- objective pieces --------------------------------------------------
    def matvec(self, x, out=None):
        """Ax = X x (loss.py:270)."""
        self._check(x, self.d, "x")
        out = self.empty_n() if out is None else self._check(out, self.n, "out")
        call("krcn_matvec", self._h, _ptr(x), _ptr(out), _stream(self.device))
        return out

    def rmatvec(self, u, out=None):
        """y = X^T u / n_global (loss.py:227,302)."""
        self._check(u, self.n, "u")
        out = self.empty_d() if out is None else self._check(out, self.d, "out")
        call("krcn_rmatvec", self._h, _ptr(u), _ptr(out), _stream(self.device))
        return out

    def weights(self, Ax, out=None):
        """w = s(1-s), s = expit(Ax) (loss.py:296-297)."""
        self._check(Ax, self.n, "Ax")
        out = self.empty_n() if out is None else self._check(out, self.n, "out")
        call("krcn_weights", self._h, _ptr(Ax), _ptr(out), _stream(self.device))
        return out

    def hvp(self, w, v, out=None, l2=0.0):
        """y = X^T (w * X v) / n + l2 v (loss.py:289-302)."""
        self._check(w, self.n, "w")
        self._check(v, self.d, "v")
        out = self.empty_d() if out is None else self._check(out, self.d, "out")
        call("krcn_hvp", self._h, _ptr(w), _ptr(v), _ptr(out), float(l2), _stream(self.device))
        return out

    def gradient(self, Ax, b, x=None, l2=0.0, out=None):
        """grad = X^T (expit(Ax) - b) / n (+ l2 x) (loss.py:223-232)."""
        self._check(Ax, self.n, "Ax")
        self._check(b, self.n, "b")
        if l2 != 0.0:
            self._check(x, self.d, "x")
        out = self.empty_d() if out is None else self._check(out, self.d, "out")
        call("krcn_gradient", self._h, _ptr(Ax), _ptr(b), _ptr(x), float(l2), _ptr(out),
             _stream(self.device))
        return out

    def loss_mean(self, Ax, b) -> float:
        """mean((1-b) Ax - logsig(Ax)) (loss.py:215-220 without the l2 term)."""
        self._check(Ax, self.n, "Ax")
        self._check(b, self.n, "b")
        out = ctypes.c_double()
        call("krcn_loss_mean", self._h, _ptr(Ax), _ptr(b), ctypes.byref(out), _stream(self.device))
        return float(out.value)

    def loss_values(self, xs, b):
        """[loss_mean(matvec(x), b) for x in xs] in one submission and one sync
        (krcn_loss_values): each value bitwise the per-iterate one."""
        self._check(b, self.n, "b")
        for i, x in enumerate(xs):
            self._check(x, self.d, f"xs[{i}]")
        k = len(xs)
        out = np.zeros(max(k, 1), dtype=np.float64)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[x.data_ptr() for x in xs])
        call("krcn_loss_values", self._h, k, ptrs, _ptr(b), out.ctypes.data_as(_lib._dp),
             _stream(self.device))
        return [float(v) for v in out[:k]]

    # -- coordinate blocks (SSCN) -------------------------------------------
    @staticmethod
    def _selection(cols):
        c = np.ascontiguousarray(np.asarray(cols).reshape(-1), dtype=np.int32)
        if not np.array_equal(c, np.asarray(cols).reshape(-1)):
            raise ValueError("cols must be integers that fit int32")
        return c, c.ctypes.data_as(ctypes.c_void_p)

    def set_coord_window(self, rows=0):
        """Rows of the LDS window of the coordinate kernels: 0 auto, else a multiple of 64."""
        call("krcn_csr_set_coord_window", self._h, int(rows))

    def coord_gradient(self, cols, Ax, b, x=None, l2=0.0):
        """Coordinates `cols` of the gradient (loss.py:234-247): numpy float64 (k,)."""
        c, cp = self._selection(cols)
        self._check(Ax, self.n, "Ax")
        self._check(b, self.n, "b")
        if l2 != 0.0:
            self._check(x, self.d, "x")
        g = np.zeros(max(len(c), 1), dtype=np.float64)
        call("krcn_coord_gradient", self._h, len(c), cp, _ptr(Ax), _ptr(b), _ptr(x), float(l2),
             g.ctypes.data_as(_lib._dp), _stream(self.device))
        return g[:len(c)]

    def coord_hessian(self, cols, Ax, l2=0.0):
        """The cols x cols block of the Hessian (loss.py:257-264): numpy float64 (k, k)."""
        c, cp = self._selection(cols)
        self._check(Ax, self.n, "Ax")
        k = len(c)
        H = np.zeros((max(k, 1), max(k, 1)), dtype=np.float64)
        call("krcn_coord_hessian", self._h, k, cp, _ptr(Ax), float(l2), H.ctypes.data_as(_lib._dp),
             _stream(self.device))
        return H[:k, :k]

    def coord_update(self, cols, delta, Ax=None, out=None):
        """Ax + X[:, cols] delta (loss.py:279-281; X[:, cols] delta when Ax is None);
        out may be Ax.  Asynchronous: cols and delta may be reused at once."""
        c, cp = self._selection(cols)
        dl = np.ascontiguousarray(np.asarray(delta).reshape(-1), dtype=np.float64)
        if len(dl) != len(c):
            raise ValueError(f"delta must have one entry per column ({len(c)}), got {len(dl)}")
        if Ax is not None:
            self._check(Ax, self.n, "Ax")
        out = self.empty_n() if out is None else self._check(out, self.n, "out")
        call("krcn_coord_update", self._h, len(c), cp, dl.ctypes.data_as(_lib._dp), _ptr(Ax), _ptr(out),
             _stream(self.device))
        return out

    # -- block products: k vectors per pass over X ---------------------------
    def _check_block(self, t, rows, k, name):
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise TypeError(f"{name} must be a torch tensor on {self.device}")
        if t.dtype != self.dtype:
            raise TypeError(f"{name} must have dtype {self.dtype}, got {t.dtype}")
        if t.dim() != 2 or t.shape[0] != rows or (k is not None and t.shape[1] != k) or not t.is_contiguous():
            want = f"({rows}, {'k' if k is None else k})"
            raise ValueError(f"{name} must be a contiguous {want} tensor, got shape {tuple(t.shape)}")
        return t

    def _block_out(self, out, rows, k):
        if out is None:
            return torch.empty((rows, k), dtype=self.dtype, device=self.device)
        return self._check_block(out, rows, k, "out")

    def matvec_block(self, V, out=None):
        """T (n, k) = X V for a (d, k) block, 1 <= k <= KRCN_BLOCK_MAX: one pass over X
        (krcn_matvec_block; scipy's csr_matvecs order).  out must not alias V."""
        k = int(self._check_block(V, self.d, None, "V").shape[1])
        out = self._block_out(out, self.n, k)
        call("krcn_matvec_block", self._h, k, _ptr(V), _ptr(out), _stream(self.device))
        return out

    def rmatvec_block(self, U, out=None):
        """Y (d, k) = X^T U / n_global for an (n, k) block (krcn_rmatvec_block)."""
        k = int(self._check_block(U, self.n, None, "U").shape[1])
        out = self._block_out(out, self.d, k)
        call("krcn_rmatvec_block", self._h, k, _ptr(U), _ptr(out), _stream(self.device))
        return out

    def hvp_block(self, w, V, l2=0.0, out=None):
        """Y[:, j] = X^T (w_j * X V[:, j]) / n + l2_j V[:, j] for a (d, k) block in two
        passes over the matrix (krcn_hvp_block).  w: (n,) weights shared by every
        column, or an (n, k) block; l2: a float or a length-k sequence."""
        k = int(self._check_block(V, self.d, None, "V").shape[1])
        if isinstance(w, torch.Tensor) and w.dim() == 2:
            w_cols = int(self._check_block(w, self.n, None, "w").shape[1])
        else:
            self._check(w, self.n, "w")
            w_cols = 1
        if np.ndim(l2) == 0:
            l2s = np.full(max(k, 1), float(l2), dtype=np.float64)
        else:
            l2s = np.ascontiguousarray(np.asarray(l2, dtype=np.float64).reshape(-1))
            if len(l2s) != k:
                raise ValueError(f"l2 must be a float or have one entry per column ({k}), got {len(l2s)}")
        out = self._block_out(out, self.d, k)
        call("krcn_hvp_block", self._h, k, _ptr(w), w_cols, _ptr(V), _ptr(out), l2s.ctypes.data_as(_lib._dp),
             _stream(self.device))
        return out

    # -- Lanczos -----------------------------------------------------------
    def lanczos(self, w, g, m, reorth=False, tol=1e-6, l2=0.0, V=None):
        """Three-term Lanczos on v -> hvp(w, v) from g (cubic.py:77-111).

        Returns (V, alphas, betas, info): V a device tensor of m rows x d (row j
        is the reference's column V[:, j]; rows >= info.m_eff are not part of
        the basis), alphas (m_eff,) and betas (m_eff-1,) numpy float64 arrays.
        """
        m = int(m)
        if m < 1:
            raise ValueError("m must be >= 1")
        self._check(w, self.n, "w")
        self._check(g, self.d, "g")
        if V is None:
            V = torch.empty((m, self.d), dtype=self.dtype, device=self.device)
        elif (V.dtype != self.dtype or V.device != self.device or not V.is_contiguous()
              or tuple(V.shape) != (m, self.d)):
            raise ValueError(f"V must be a contiguous ({m}, {self.d}) {self.dtype} tensor on {self.device}")
        if reorth and m > self._reorth_m:
            self.reserve(m, reorth=True)   # before the recurrence, not inside it
        # host result buffers reused across calls (w8a's m = 10 calls are
        # ~165 us each: the wrapper's own allocations showed up); the
        # returned arrays are copies
        if self._lz_bufs is None or self._lz_bufs[0].size < m:
            cap = max(m, 64)
            al_b, be_b = np.zeros(cap, dtype=np.float64), np.zeros(cap, dtype=np.float64)
            self._lz_bufs = (al_b, be_b, al_b.ctypes.data_as(_lib._dp), be_b.ctypes.data_as(_lib._dp))
        al_b, be_b, al_p, be_p = self._lz_bufs
        info = _lib.LanczosInfo()
        st = self._fn_lanczos(self._h, _ptr(w), _ptr(g), m, int(bool(reorth)), float(tol), float(l2),
                              _ptr(V), al_p, be_p, ctypes.byref(info), _stream(self.device))
        if st != _lib.KRCN_OK:
            msg = _lib.load().krcn_last_error_string()
            raise _lib.KrcnError(st, "krcn_lanczos", msg.decode() if msg else "")
        me = info.m_eff
        return V, al_b[:me].copy(), be_b[:max(me - 1, 0)].copy(), info

    def cgs2(self, V, z, k=None):
        """z <- (I - Vk^T Vk)(I - Vk^T Vk) z in place over the first k rows of V
        (krcn_cgs2: the reorthogonalisation of lanczos(reorth=True) on a
        caller's basis, which need not be orthonormal).  V is a contiguous
        (rows >= k, d) tensor and z a contiguous d-vector; either may be a view
        into a larger buffer.  Returns (norm2, path): ||z2||^2 as the
        recurrence sums it, and 1 for the 1 KiB-piece sweeps, 0 for the batched."""
        if (not isinstance(V, torch.Tensor) or V.dtype != self.dtype or V.device != self.device
                or V.dim() != 2 or V.shape[1] != self.d or not V.is_contiguous()):
            raise ValueError(f"V must be a contiguous (rows, {self.d}) {self.dtype} tensor on {self.device}")
        k = V.shape[0] if k is None else int(k)
        if k < 1 or k > V.shape[0]:
            raise ValueError(f"k = {k} outside [1, {V.shape[0]}]")
        self._check(z, self.d, "z")
        norm2, path = ctypes.c_double(), ctypes.c_int(-1)
        call("krcn_cgs2", self._h, k, _ptr(V), _ptr(z), ctypes.byref(norm2), ctypes.byref(path),
             _stream(self.device))
        self._reorth_m = max(self._reorth_m, k + 1)
        return float(norm2.value), int(path.value)

    # -- batched Lanczos: k recurrences in lockstep over the block HVP --------
    def lanczos_block(self, w, G, m, tol=1e-6, l2=0.0, V=None):
        """k independent Lanczos recurrences over one X, advanced together
        (krcn_lanczos_block): column c is `lanczos(w_c, G[:, c], m, l2=l2_c)`.

        w: (n,) weights shared by every column, or an (n, k) block; G: (d, k)
        start block; l2: a float or a length-k sequence.  Returns (V, alphas,
        betas, infos): V a device tensor (m, d, k), slab j column c the
        reference's V[:, j] of problem c and zero where problem c has no basis
        vector; alphas, betas, infos length-k lists, truncated per column as
        `lanczos` truncates."""
        m = int(m)
        if m < 1:
            raise ValueError("m must be >= 1")
        k = int(self._check_block(G, self.d, None, "G").shape[1])
        if isinstance(w, torch.Tensor) and w.dim() == 2:
            w_cols = int(self._check_block(w, self.n, None, "w").shape[1])
        else:
            self._check(w, self.n, "w")
            w_cols = 1
        if np.ndim(l2) == 0:
            l2s = np.full(max(k, 1), float(l2), dtype=np.float64)
        else:
            l2s = np.ascontiguousarray(np.asarray(l2, dtype=np.float64).reshape(-1))
            if len(l2s) != k:
                raise ValueError(f"l2 must be a float or have one entry per column ({k}), got {len(l2s)}")
        if V is None:
            V = torch.empty((m, self.d, k), dtype=self.dtype, device=self.device)
        elif (not isinstance(V, torch.Tensor) or V.dtype != self.dtype or V.device != self.device
              or not V.is_contiguous() or tuple(V.shape) != (m, self.d, k)):
            raise ValueError(f"V must be a contiguous ({m}, {self.d}, {k}) {self.dtype} tensor on {self.device}")
        mb = max(m - 1, 1)
        al = np.zeros((max(k, 1), m), dtype=np.float64)
        be = np.zeros((max(k, 1), mb), dtype=np.float64)
        infos = (_lib.LanczosInfo * max(k, 1))()
        call("krcn_lanczos_block", self._h, k, _ptr(w), w_cols, _ptr(G), m, float(tol), l2s.ctypes.data_as(_lib._dp),
             _ptr(V), al.ctypes.data_as(_lib._dp), be.ctypes.data_as(_lib._dp), infos, _stream(self.device))
        alphas = [al[c, :infos[c].m_eff].copy() for c in range(k)]
        betas = [be[c, :max(infos[c].m_eff - 1, 0)].copy() for c in range(k)]
        return V, alphas, betas, [infos[c] for c in range(k)]

    def basis_combine_block(self, V, S, X0, out=None):
        """X0[:, c] + sum_j V[j, :, c] S[j, c] over the slabs of a lanczos_block
        basis (krcn_basis_combine_block).  S: (m', k) host coefficients, m' <=
        V.shape[0], zero-padded past a column's m_eff."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        if S.ndim != 2:
            raise ValueError("S must be (m, k)")
        mm, k = int(S.shape[0]), int(S.shape[1])
        self._check_block(X0, self.d, k, "X0")
        if (not isinstance(V, torch.Tensor) or V.dtype != self.dtype or V.device != self.device or V.dim() != 3
                or not V.is_contiguous() or V.shape[0] < mm or tuple(V.shape[1:]) != (self.d, k)):
            raise ValueError(f"V must be a contiguous (>= {mm}, {self.d}, {k}) {self.dtype} tensor on {self.device}")
        out = self._block_out(out, self.d, k)
        call("krcn_basis_combine_block", self._h, k, mm, _ptr(V), S.ctypes.data_as(_lib._dp), _ptr(X0), _ptr(out),
             _stream(self.device))
        return out

    def weights_block(self, AX, out=None):
        """W = s (1 - s), s = expit(AX), for an (n, k) block AX = X xs
        (krcn_weights_block): `weights` column by column."""
        k = int(self._check_block(AX, self.n, None, "AX").shape[1])
        out = self._block_out(out, self.n, k)
        call("krcn_weights_block", self._h, k, _ptr(AX), _ptr(out), _stream(self.device))
        return out

    def cg_solve(self, w, b, shift=0.0, rtol=1e-5, maxiter=None, out=None):
        """x ~= (H + shift I)^{-1} b, H = X^T diag(w) X / n, by device conjugate
        gradients with scipy.sparse.linalg.cg's loop and stopping rule (x0 = 0,
        stop when ||r|| < rtol ||b||, maxiter default 10 d).  Returns (x, info)."""
        self._check(w, self.n, "w")
        self._check(b, self.d, "b")
        out = self.empty_d() if out is None else self._check(out, self.d, "out")
        maxiter = 10 * self.d if maxiter is None else int(maxiter)
        info = _lib.CgInfo()
        call("krcn_cg_solve", self._h, _ptr(w), _ptr(b), float(shift), float(rtol), maxiter, _ptr(out),
             ctypes.byref(info), _stream(self.device))
        return out, info

    def basis_combine(self, V, s, x, out=None):
        """x + V^T s over the first len(s) basis rows (cubic.py:291)."""
        s = np.ascontiguousarray(s, dtype=np.float64)
        self._check(x, self.d, "x")
        if V.dim() != 2 or V.shape[1] != self.d or V.shape[0] < len(s):
            raise ValueError("V must be (>= len(s)) x d")
        out = self.empty_d() if out is None else self._check(out, self.d, "out")
        call("krcn_basis_combine", self._h, len(s), _ptr(V), s.ctypes.data_as(_lib._dp), _ptr(x),
             _ptr(out), _stream(self.device))
        return out

    # -- the Krylov-CRN step on the device -----------------------------------
    def cubic_tridiag(self, alphas, betas, gnorm, M, r0=0.1, eps=1e-8, it_max=100):
        """The cubic subproblem over T = tridiag(betas, alphas, betas) with
        g = gnorm e1, solved on the device in fp64 (krcn_cubic_tridiag; what
        optimizer.cubic.cubic_solver_root_tridiag computes on the host).
        Returns (s, info): s a numpy (m,) array, info a _lib.CrnInfo whose
        solver_it / solver_status / lam / model_decrease / reg_coef are set
        (status 0 ok, 1 T + lam I not positive definite, 2 derivative zero,
        3 it_max reached with the last iterate returned)."""
        al = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
        be = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
        m = len(al)
        if len(be) != max(m - 1, 0):
            raise ValueError("betas must have len(alphas) - 1 entries")
        s = np.zeros(max(m, 1), dtype=np.float64)
        info = _lib.CrnInfo()
        call("krcn_cubic_tridiag", self._h, m, al.ctypes.data_as(_lib._dp),
             be.ctypes.data_as(_lib._dp) if m > 1 else None, float(gnorm), float(M), float(r0), float(eps),
             int(it_max), s.ctypes.data_as(_lib._dp), ctypes.byref(info), _stream(self.device))
        return s[:m], info

    def crn_step(self, x, b, value, m, reg_coef, Ax=None, V=None, reorth=False, tol=1e-6, l2=0.0, ls_beta=0.5,
                 r0=0.1, solver_eps=1e-8, solver_it_max=100, max_trials=20, x_new=None, Ax_new=None):
        """One Krylov-CRN step from x with f(x) = value behind one library call
        (krcn_crn_step): gradient, weights, Lanczos, then the backtracking line
        search with the subproblem and the accept / reject test on the device.
        Ax is X x when the caller has it.  Returns (x_new, Ax_new, alphas,
        betas, info): the iterate the step keeps and its product with X (device
        tensors), the recurrence's alphas / betas as lanczos() returns them,
        and a _lib.CrnInfo (accepted, trials, solver_it, solver_status,
        reg_coef, lam, model_decrease, value_new, dx_norm, lanczos)."""
        m = int(m)
        if m < 1:
            raise ValueError("m must be >= 1")
        self._check(x, self.d, "x")
        self._check(b, self.n, "b")
        if Ax is not None:
            self._check(Ax, self.n, "Ax")
        if V is None:
            V = torch.empty((m, self.d), dtype=self.dtype, device=self.device)
        elif (V.dtype != self.dtype or V.device != self.device or not V.is_contiguous()
              or tuple(V.shape) != (m, self.d)):
            raise ValueError(f"V must be a contiguous ({m}, {self.d}) {self.dtype} tensor on {self.device}")
        x_new = self.empty_d() if x_new is None else self._check(x_new, self.d, "x_new")
        Ax_new = self.empty_n() if Ax_new is None else self._check(Ax_new, self.n, "Ax_new")
        if reorth and m > self._reorth_m and self.shard_mode == _lib.KRCN_SHARD_NONE:
            self.reserve(m, reorth=True)
        al = np.zeros(m, dtype=np.float64)
        be = np.zeros(max(m - 1, 1), dtype=np.float64)
        info = _lib.CrnInfo()
        call("krcn_crn_step", self._h, _ptr(x), _ptr(b), _ptr(Ax), float(value), m, int(bool(reorth)), float(tol),
             float(l2), float(reg_coef), float(ls_beta), float(r0), float(solver_eps), int(solver_it_max),
             int(max_trials), _ptr(V), _ptr(x_new), _ptr(Ax_new), al.ctypes.data_as(_lib._dp),
             be.ctypes.data_as(_lib._dp), ctypes.byref(info), _stream(self.device))
        me = info.lanczos.m_eff
        return x_new, Ax_new, al[:me], be[:max(me - 1, 0)], info

    # -- the SSCN step on the device -------------------------------------------
    def cubic_dense(self, H, g, M, r0=0.1, eps=1e-8, it_max=100):
        """The cubic subproblem over a dense symmetric k x k block H and a
        general g, 1 <= k <= KRCN_SSCN_MAX, solved on the device in fp64
        (krcn_cubic_dense; what optimizer.cubic.cubic_solver_root computes on
        the host).  Only the upper triangle of H is read.  Returns (s, info) as
        `cubic_tridiag`: status 1 means H + lam I was not positive definite."""
        Hd, gd, k = self._dense_block(H, g)
        s = np.zeros(max(k, 1), dtype=np.float64)
        info = _lib.CrnInfo()
        call("krcn_cubic_dense", self._h, k, Hd.ctypes.data_as(_lib._dp), gd.ctypes.data_as(_lib._dp), float(M),
             float(r0), float(eps), int(it_max), s.ctypes.data_as(_lib._dp), ctypes.byref(info),
             _stream(self.device))
        return s[:k], info

    @staticmethod
    def dense_tridiag_geometry(k):
        """(column launches, workspace bytes) of the tridiagonal reduction of a
        k-column block (krcn_dense_tridiag_geometry; host arithmetic only)."""
        launches, ws = ctypes.c_int64(0), ctypes.c_int64(0)
        call("krcn_dense_tridiag_geometry", int(k), ctypes.byref(launches), ctypes.byref(ws))
        return launches.value, ws.value

    @staticmethod
    def _dense_block(H, g):
        Hd = np.ascontiguousarray(H.toarray() if hasattr(H, "toarray") else H, dtype=np.float64)
        gd = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
        k = len(gd)
        if Hd.shape != (k, k):
            raise ValueError(f"H must be ({k}, {k}), got {Hd.shape}")
        return Hd, gd, k

    def dense_tridiag(self, H, g, want_q=False):
        """The Householder reduction behind `cubic_dense_tridiag` alone
        (krcn_dense_tridiag), 1 <= k <= KRCN_SSCN_TRIDIAG_MAX: H = Q T Q^T with
        T = tridiag(betas[1:], alphas, betas[1:]) and g = betas[0] Q e1
        (betas[0] is the signed ||g||).  Only the upper triangle of H is read.
        Returns (alphas, betas, Q); Q is None unless want_q (a test path)."""
        Hd, gd, k = self._dense_block(H, g)
        n = max(k, 1)
        al = np.full(n, np.nan)
        be = np.full(n, np.nan)
        Q = np.full((n, n), np.nan) if want_q else None
        call("krcn_dense_tridiag", self._h, k, Hd.ctypes.data_as(_lib._dp), gd.ctypes.data_as(_lib._dp),
             al.ctypes.data_as(_lib._dp), be.ctypes.data_as(_lib._dp),
             Q.ctypes.data_as(_lib._dp) if want_q else None, _stream(self.device))
        return al[:k], be[:k], (Q[:k, :k] if want_q else None)

    def cubic_dense_tridiag(self, H, g, M, r0=0.1, eps=1e-8, it_max=100):
        """`cubic_dense` for 1 <= k <= KRCN_SSCN_TRIDIAG_MAX over one
        tridiagonal reduction of H (krcn_cubic_dense_tridiag): the reduction,
        the tridiagonal subproblem of `cubic_tridiag`, and s = Q s_T.  Returns
        (s, info) as `cubic_dense`."""
        Hd, gd, k = self._dense_block(H, g)
        s = np.full(max(k, 1), np.nan)
        info = _lib.CrnInfo()
        call("krcn_cubic_dense_tridiag", self._h, k, Hd.ctypes.data_as(_lib._dp), gd.ctypes.data_as(_lib._dp),
             float(M), float(r0), float(eps), int(it_max), s.ctypes.data_as(_lib._dp), ctypes.byref(info),
             _stream(self.device))
        return s[:k], info

    def sscn_step(self, cols, x, b, value, reg_coef, Ax=None, l2=0.0, ls_beta=0.5, r0=0.1,
                  solver_eps=float(np.finfo(float).eps), solver_it_max=100, max_trials=20, x_new=None, Ax_new=None,
                  subproblem="cholesky"):
        """One SSCN step from x with f(x) = value over the distinct columns
        `cols` behind one library call (krcn_sscn_step): coordinate gradient
        and Hessian block, then the backtracking line search with the dense
        subproblem, the coordinate update of Ax and the accept / reject test
        on the device.  Ax is X x when the caller has it.  Returns (x_new,
        Ax_new, info): the iterate the step keeps, its product with X, and a
        _lib.CrnInfo (accepted, trials, solver_it, solver_status, reg_coef,
        lam, model_decrease, value_new, dx_norm = ||s||).
        subproblem: "cholesky" (krcn_sscn_step, up to KRCN_SSCN_MAX columns: a
        Cholesky factorisation per lam) or "tridiag" (krcn_sscn_step_tridiag, up
        to KRCN_SSCN_TRIDIAG_MAX: one tridiagonal reduction per step)."""
        if subproblem not in ("cholesky", "tridiag"):
            raise ValueError(f'subproblem must be "cholesky" or "tridiag", got {subproblem!r}')
        c, cp = self._selection(cols)
        self._check(x, self.d, "x")
        self._check(b, self.n, "b")
        if Ax is not None:
            self._check(Ax, self.n, "Ax")
        x_new = self.empty_d() if x_new is None else self._check(x_new, self.d, "x_new")
        Ax_new = self.empty_n() if Ax_new is None else self._check(Ax_new, self.n, "Ax_new")
        info = _lib.CrnInfo()
        fn = "krcn_sscn_step" if subproblem == "cholesky" else "krcn_sscn_step_tridiag"
        call(fn, self._h, len(c), cp, _ptr(x), _ptr(b), _ptr(Ax), float(value), float(l2), float(reg_coef),
             float(ls_beta), float(r0), float(solver_eps), int(solver_it_max), int(max_trials), _ptr(x_new),
             _ptr(Ax_new), ctypes.byref(info), _stream(self.device))
        return x_new, Ax_new, info

    # -- the full-space cubic subproblem on the device --------------------------
    def cubic_cg(self, w, g, M, l2=0.0, r0=0.1, eps=1e-8, it_max=100, cg_rtol=None, cg_maxiter=None, out=None):
        """argmin_s <g,s> + 1/2 s^T H s + M/3 ||s||^3 for H = X^T diag(w) X / n
        + l2 I behind one library call (krcn_cubic_cg): scipy's scalar Newton
        on phi(lam) from r0 with every (H + lam I)^{-1} applied by `cg_solve`'s
        conjugate gradients (rtol cg_rtol, default eps; at most cg_maxiter
        updates per solve, default 10 d), the decisions taken on the device.
        Returns (s, info): s a device d-vector (zeros when the solve failed),
        info a _lib.CubicCgInfo (solver_it, solver_status — 0 ok, 1 not
        positive definite, 2 derivative zero, 3 it_max reached with the last
        iterate returned, 4 non-finite —, cg_solves, cg_unconverged,
        cg_iterations, ticks, reg_coef, lam, model_decrease, s_norm)."""
        self._check(w, self.n, "w")
        self._check(g, self.d, "g")
        out = self.empty_d() if out is None else self._check(out, self.d, "out")
        info = _lib.CubicCgInfo()
        call("krcn_cubic_cg", self._h, _ptr(w), _ptr(g), float(l2), float(M), float(r0), float(eps), int(it_max),
             float(eps if cg_rtol is None else cg_rtol), 0 if cg_maxiter is None else int(cg_maxiter), _ptr(out),
             ctypes.byref(info), _stream(self.device))
        return out, info

    # -- the dense Hessian as one Gram product ---------------------------------
    def set_gram_split(self, split=0):
        """Workgroups per output tile of hessian_gram along the summed index
        (krcn_csr_set_gram_split): 0 the rule of gram_geometry, else 1..256."""
        call("krcn_csr_set_gram_split", self._h, int(split))

    def hessian_gram(self, w, l2=0.0, out=None):
        """H = X^T diag(w) X / n + l2 I (loss.py:249-255) as one weighted Gram
        product over the dense image of X^T, in fp64 on the matrix instruction
        (krcn_hessian_gram): a device (d, d) float64 tensor, exactly symmetric,
        the same bytes on every call.  Needs a dense pass 2 (set_format(5) or
        set_pass_format(2, 5)); the library's KRCN_ERR_UNSUPPORTED is raised
        otherwise.  w: the device n-vector `weights` returns."""
        self._check(w, self.n, "w")
        if out is None:
            out = torch.empty((self.d, self.d), dtype=torch.float64, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float64
              or tuple(out.shape) != (self.d, self.d) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous ({self.d}, {self.d}) float64 tensor on {self.device}")
        # an empty tensor has no address: n == 0 never reads w, d == 0 never writes H
        wp = _ptr(w) if self.n else _ptr(self.indptr)
        Hp = _ptr(out) if self.d else _ptr(self.indptr)
        call("krcn_hessian_gram", self._h, wp, float(l2), Hp, _stream(self.device))
        return out

    # -- the batched Krylov-CRN step: k problems over one X --------------------
    @staticmethod
    def _per_column(v, k, name):
        """A float or a length-k sequence as k contiguous float64."""
        if np.ndim(v) == 0:
            return np.full(max(k, 1), float(v), dtype=np.float64)
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
        if len(a) != k:
            raise ValueError(f"{name} must be a float or have one entry per column ({k}), got {len(a)}")
        return a

    def _labels(self, b, k):
        """b as krcn_*_block takes it: an n-vector (b_cols = 1) or an (n, k) block (b_cols = k)."""
        if isinstance(b, torch.Tensor) and b.dim() == 2:
            self._check_block(b, self.n, k, "b")
            return k
        self._check(b, self.n, "b")
        return 1

    def gradient_block(self, AX, b, X=None, l2=0.0, out=None):
        """G[:, c] = X^T (expit(AX[:, c]) - b_c) / n + l2_c X[:, c] for an (n, k)
        block AX (krcn_gradient_block): `gradient` column by column.  b: (n,)
        labels shared by every column, or an (n, k) block of 0/1 labels; l2: a
        float or a length-k sequence; X: the (d, k) iterates, needed where some
        l2_c != 0."""
        k = int(self._check_block(AX, self.n, None, "AX").shape[1])
        b_cols = self._labels(b, k)
        l2s = self._per_column(l2, k, "l2")
        if l2s.any():
            self._check_block(X, self.d, k, "X")
        out = self._block_out(out, self.d, k)
        call("krcn_gradient_block", self._h, k, _ptr(AX), _ptr(b), b_cols, _ptr(X), l2s.ctypes.data_as(_lib._dp),
             _ptr(out), _stream(self.device))
        return out

    def value_block(self, AX, b, X=None, l2=0.0):
        """f_c = mean((1 - b_c) a - logsig(a)) + l2_c / 2 ||X[:, c]||^2 over a =
        AX[:, c] (krcn_value_block): a numpy (k,) array, one loss value per column."""
        k = int(self._check_block(AX, self.n, None, "AX").shape[1])
        b_cols = self._labels(b, k)
        l2s = self._per_column(l2, k, "l2")
        if l2s.any():
            self._check_block(X, self.d, k, "X")
        out = np.zeros(max(k, 1), dtype=np.float64)
        call("krcn_value_block", self._h, k, _ptr(AX), _ptr(b), b_cols, _ptr(X), l2s.ctypes.data_as(_lib._dp),
             out.ctypes.data_as(_lib._dp), _stream(self.device))
        return out[:k]

    def cubic_tridiag_block(self, alphas, betas, gnorm, M, r0=0.1, eps=1e-8, it_max=100):
        """k subproblems of `cubic_tridiag` in one launch (krcn_cubic_tridiag_block).
        alphas / betas: length-k lists of arrays (column c has len(alphas[c]) =
        m_eff_c entries and m_eff_c - 1 betas); gnorm, M, r0: floats or length-k
        sequences.  Returns (s, infos): s a list of numpy (m_eff_c,) arrays,
        infos a list of _lib.CrnInfo; per column bitwise `cubic_tridiag`."""
        k = len(alphas)
        if len(betas) != k:
            raise ValueError("alphas and betas must list the same number of columns")
        als = [np.asarray(a, dtype=np.float64).reshape(-1) for a in alphas]
        bes = [np.asarray(a, dtype=np.float64).reshape(-1) for a in betas]
        m = max([len(a) for a in als] + [1])
        mb = max(m - 1, 1)
        al = np.zeros((max(k, 1), m), dtype=np.float64)
        be = np.zeros((max(k, 1), mb), dtype=np.float64)
        m_eff = np.ones(max(k, 1), dtype=np.int32)
        for c in range(k):
            if len(als[c]) < 1 or len(bes[c]) != len(als[c]) - 1:
                raise ValueError(f"column {c}: betas must have len(alphas) - 1 entries and alphas at least one")
            m_eff[c] = len(als[c])
            al[c, :len(als[c])] = als[c]
            be[c, :len(bes[c])] = bes[c]
        gn, Ms, r0s = (self._per_column(v, k, nm) for v, nm in ((gnorm, "gnorm"), (M, "M"), (r0, "r0")))
        s = np.zeros((max(k, 1), m), dtype=np.float64)
        infos = (_lib.CrnInfo * max(k, 1))()
        dp = _lib._dp
        call("krcn_cubic_tridiag_block", self._h, k, m, m_eff.ctypes.data_as(_lib._ip), al.ctypes.data_as(dp),
             be.ctypes.data_as(dp), gn.ctypes.data_as(dp), Ms.ctypes.data_as(dp), r0s.ctypes.data_as(dp), float(eps),
             int(it_max), s.ctypes.data_as(dp), infos, _stream(self.device))
        return [s[c, :m_eff[c]].copy() for c in range(k)], [infos[c] for c in range(k)]

    def crn_step_block(self, X, b, values, m, reg_coef, AX=None, V=None, active=None, tol=1e-6, l2=0.0, ls_beta=0.5,
                       r0=0.1, solver_eps=1e-8, solver_it_max=100, max_trials=20, X_new=None, AX_new=None):
        """One Krylov-CRN step of k problems over this matrix behind one library
        call (krcn_crn_step_block): column c is `crn_step(X[:, c], b_c,
        values[c], m, reg_coef[c], l2=l2[c], r0=r0[c])` with the line search
        decided per column on the device.  X: (d, k) iterates; b: (n,) labels or
        an (n, k) block; values: length-k f_c(x_c); reg_coef, l2, r0: floats or
        length-k sequences; AX: X X when the caller has it; active: length-k
        flags (a column with a false flag is copied through unchanged).  Returns
        (X_new, AX_new, alphas, betas, infos): device (d, k) and (n, k) blocks,
        the recurrences' alphas / betas as lanczos_block() returns them, and a
        list of _lib.CrnInfo."""
        m = int(m)
        if m < 1:
            raise ValueError("m must be >= 1")
        k = int(self._check_block(X, self.d, None, "X").shape[1])
        b_cols = self._labels(b, k)
        if AX is not None:
            self._check_block(AX, self.n, k, "AX")
        vals = self._per_column(values, k, "values")
        regs = self._per_column(reg_coef, k, "reg_coef")
        l2s = self._per_column(l2, k, "l2")
        r0s = self._per_column(r0, k, "r0")
        act = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, dtype=np.int32)
            if len(act) != k:
                raise ValueError(f"active must have one entry per column ({k}), got {len(act)}")
        if V is None:
            V = torch.empty((m, self.d, k), dtype=self.dtype, device=self.device)
        elif (not isinstance(V, torch.Tensor) or V.dtype != self.dtype or V.device != self.device
              or not V.is_contiguous() or tuple(V.shape) != (m, self.d, k)):
            raise ValueError(f"V must be a contiguous ({m}, {self.d}, {k}) {self.dtype} tensor on {self.device}")
        X_new = self._block_out(X_new, self.d, k)
        AX_new = self._block_out(AX_new, self.n, k)
        mb = max(m - 1, 1)
        al = np.zeros((max(k, 1), m), dtype=np.float64)
        be = np.zeros((max(k, 1), mb), dtype=np.float64)
        infos = (_lib.CrnInfo * max(k, 1))()
        dp = _lib._dp
        call("krcn_crn_step_block", self._h, k, _ptr(X), _ptr(b), b_cols, _ptr(AX), vals.ctypes.data_as(dp),
             None if act is None else act.ctypes.data_as(_lib._ip), m, float(tol), l2s.ctypes.data_as(dp),
             regs.ctypes.data_as(dp), float(ls_beta), r0s.ctypes.data_as(dp), float(solver_eps), int(solver_it_max),
             int(max_trials), _ptr(V), _ptr(X_new), _ptr(AX_new), al.ctypes.data_as(dp), be.ctypes.data_as(dp), infos,
             _stream(self.device))
        alphas = [al[c, :infos[c].lanczos.m_eff].copy() for c in range(k)]
        betas = [be[c, :max(infos[c].lanczos.m_eff - 1, 0)].copy() for c in range(k)]
        return X_new, AX_new, alphas, betas, [infos[c] for c in range(k)]

    # -- vector helpers ----------------------------------------------------
    def _space_len(self, space):
        return self.n if space == _lib.KRCN_SPACE_N else self.d

    def dot(self, a, b, space=_lib.KRCN_SPACE_D) -> float:
        ln = self._space_len(space)
        self._check(a, ln, "a")
        self._check(b, ln, "b")
        out = ctypes.c_double()
        call("krcn_dot", self._h, space, _ptr(a), _ptr(b), ctypes.byref(out), _stream(self.device))
        return float(out.value)

    def diff_norm(self, a, b=None, space=_lib.KRCN_SPACE_D) -> float:
        ln = self._space_len(space)
        self._check(a, ln, "a")
        if b is not None:
            self._check(b, ln, "b")
        out = ctypes.c_double()
        call("krcn_diff_norm", self._h, space, _ptr(a), _ptr(b), ctypes.byref(out),
             _stream(self.device))
        return float(out.value)

    # -- profiling ---------------------------------------------------------
    def prof_enable(self, on=True):
        call("krcn_prof_enable", self._h, int(bool(on)))

    def prof_read(self):
        """{'count', 'pass1_ms' (with its slice combine), 'pass2_ms', 'hvp_ms',
        'pass1_kernel_ms', 'combine_ms'} accumulated since enable/last read."""
        buf = (ctypes.c_double * 8)()
        call("krcn_prof_read", self._h, buf)
        return {"count": int(buf[0]), "pass1_ms": buf[1], "pass2_ms": buf[3], "hvp_ms": buf[5],
                "pass1_kernel_ms": buf[6], "combine_ms": buf[7]}
