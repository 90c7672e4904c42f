"""krcn_cgs2 (the reorthogonalisation sweeps of krcn_lanczos(reorth=1), run on a
caller's basis) one call at a time against oracle/krcn_oracle.py: cgs2_apply,
on bases that are NOT orthonormal, at the size edges of krcn_cgs2.hpp.

Inside a recurrence V is orthonormal, so what one pass drops the other removes
(or is O(eps) already) and alphas, betas and V V^T - I stay inside their
tolerances.  Here V has entries N(0, 1) / sqrt(d): every sweep changes z at
O(1), and a row, column, chunk or slab that a sweep drops or misplaces shows in
z2 at 1e5 times the bound or more (tests/test_oracle_cgs2.py asserts that on the
reference alone, and holds the shapes and inputs of this file).

Every case is one call on a handle built from a 1 x d matrix with one nonzero
(its content is irrelevant), with V and z inside larger buffers between
sentinels, and asserts, in this order: the path the call reports (1: the 1 KiB-
piece sweeps, 0: the batched ones), so that no case silently tests the other
one; V and every sentinel bitwise unchanged; z2 within cgs2_bound of the
reference component by component and ||z2||^2 within its bound; a second
identical call bitwise equal in z2 and ||z2||^2 (fixed summation order, and
with more than one row range: the last arrival reset the ticket counters).
Rows that are not whole 16-byte vectors (odd d in fp64, d % 4 != 0 in fp32)
take the batched path by themselves; an aligned shape takes it when z starts
one element into its buffer, and then both paths run on the same V and z and
are compared with each other at the same bound.

The bound (oracle/krcn_oracle.py: cgs2_bound) is the standard inner-product
bound with gamma = (d + k + 8) 2^-53, plus, in fp32, one ulp of z2 and a one-ulp
flip of the stored z1 carried through pass 2.  Measured error / bound on an
MI355X, ROCm 7.0 (largest over the cases of a path and dtype, ||z2||^2 in
brackets; every case prints its own as MEASURED):
  batched fp64  0.023 (0.032)      1 KiB fp64  0.036 (0.012)
  batched fp32  0     (3.2e-10)    1 KiB fp32  0     (3.2e-10)
  the two paths against each other: fp64 0.026, fp32 0
The largest ratios come from d <= 2, where the bound is smallest; at d >= 8191
they are at most 1.4e-4 (the bound grows with d + k, the error of these sums
hardly).  In fp32 every z2 is bitwise the reference's: the double sums err by
1e-9 of a float32 ulp, so a rounding falls on the other side about once in
1e8 components.  The two recurrence cases: alphas / betas 1.6e-14 / 1.5e-14
(d = 8193, m = 300) and 3.0e-15 / 4.1e-15 (two column shards) against 1e-10.

The edges (krcn_cgs2.hpp, krcn_lanczos_impl.hpp reorth_cgs2):
  batched   k = 1, 8 | 9, 16 | 17, 32 | 33, 64 | 65, 128 | 129: cgs_unroll's
            U = 1, 1 | 2, 2 | 4, 4 | 8, 8 | 16, and cgs_norm_unroll's (8 row
            groups) one step earlier; 256 | 257, 512 | 513: the 256-row trips
            of the U = 16 loops, and the last cached / first uncached launch of
            k_cgs_update_dots (k * 36 * sizeof(T) <= 73,728: k <= 256 in fp64,
            512 in fp32; the cached launches at those k ask for 78,080 bytes of
            dynamic LDS); 2043: the largest k, all at d = 33 (two 32-column
            slabs, fewer than k_cgs_coeffs' 64 slab groups);
            d = 1, 31 | 32 | 33, 63 | 64 | 65 around the 32-column slab of the
            update and the 64-column slab of the norm sweep;
            cgs_rd_chunks: C = 1, 2, 3, 2, 1 (CHUNK_CASES: the staged partials
            of cgs_load_h for C > 1, and C k <= 1024 at 3 * 341 = 1023);
            2050 slabs at d = 65,569: k_cgs_coeffs' second round of loads;
            2049 slabs of 64 columns at d = 131,073: k_cgs_update_norm's
            grid-stride (V is 9.4 MB in fp64).
  1 KiB     k = 1, 4 | 5, 8 | 9, 16 | 17, 32 | 33: cgs_col_unroll's U = 1, 1 |
            2, 2 | 4, 4 | 8, 8 and then the NB loop's second batch (32 rows a
            batch at U = 8) with its early break; 64 | 65: batches 2 | 3;
            256 | 257: Q = 1 | 2 row ranges (the in-launch hand-off); 513: 3;
            1792 | 1793: 7 | 8, the first trip of the 8-at-a-time combine;
            2043: 8 again with a short last range; all at d = 64 E + E (two
            column groups, the second holding one vector);
            d = E, 64 E - E, 64 E, 64 E + E: column groups;
            rows of nv = d / E = 256, 1793, 2049, 3841, 4097, 65,537 vectors:
            C = 1, 8, 9, 16 chunks at S = 1 (the prologue's rounds of 8 loads),
            C = 9 at S = 2, and C = 17 at S = 16 (past kCgsRdChunksV).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
import krcn_oracle as O
import test_oracle_cgs2 as C
from conftest import rel_err
from krcn import _lib
from krcn import dist as kdist
from krcn import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
BITS = {"fp64": torch.int64, "fp32": torch.int32}
PAD = 64            # sentinel elements on either side (whole 16-byte vectors in both dtypes)
SENTINEL = 3.0e30   # finite in float32; would swamp any sum that reached it


def handle(d, prec):
    A = sp.csr_matrix((np.ones(1), (np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32))), shape=(1, d))
    return krcn.DeviceCSR(A, dtype=TORCH[prec])


def place(a, prec, lead=0):
    """A flat device buffer PAD + lead sentinels | a | PAD sentinels, and the view of a inside it."""
    buf = torch.full((PAD + lead + a.size + PAD,), SENTINEL, dtype=TORCH[prec], device=DEV)
    view = buf[PAD + lead:PAD + lead + a.size]
    view.copy_(torch.from_numpy(np.array(a).ravel()))   # (a copy: the cases' arrays are read-only)
    return buf, view.view(a.shape)


def bits(t, prec):
    return t.view(BITS[prec])


def run(X, d, k, prec, want_path, lead=0):
    """One krcn_cgs2 call on the case's inputs with z `lead` elements off 16-byte alignment; every assertion of
    the module docstring.  Returns z2 (numpy) and error / bound, norm2 error / bound."""
    Vh, zh = C.inputs(d, k, prec)
    bufV, V = place(Vh, prec)
    bufz, z = place(zh, prec, lead)
    assert V.data_ptr() % 16 == 0
    assert (z.data_ptr() % 16 == 0) == (lead == 0)
    V0, z0 = bufV.clone(), bufz.clone()
    n2, path = X.cgs2(V, z)
    assert path == want_path, f"ran path {path}, this case is about path {want_path}"
    assert torch.equal(bits(bufV, prec), bits(V0, prec)), "V or a sentinel around it was written"
    for part in (slice(0, PAD + lead), slice(PAD + lead + d, None)):
        assert torch.equal(bits(bufz[part], prec), bits(z0[part], prec)), "a sentinel around z was written"
    got = z.cpu().numpy().copy()
    z1, z2, n2_ref, bound, n2_bound = C.reference(d, k, prec)
    r, rn = C.ratio(got, z2, bound), abs(n2 - float(n2_ref)) / n2_bound
    print(f"MEASURED path {path} {prec} d = {d} k = {k}: error / bound {r:.3g}, norm2 {rn:.3g}")
    assert np.isfinite(got).all()
    assert r <= 1.0, f"z2 off by {r:.3g} of the bound"
    assert rn <= 1.0, f"||z2||^2 = {n2!r} against {float(n2_ref)!r}: {rn:.3g} of the bound"
    bufz.copy_(z0)
    n2b, pathb = X.cgs2(V, z)
    assert pathb == path
    assert n2b == n2 and torch.equal(bits(z, prec), bits(torch.from_numpy(got).to(DEV), prec)), "not deterministic"
    return got, r, rn


def both_paths(X, d, k, prec):
    """An aligned shape: the 1 KiB-piece sweeps, then the batched ones on the same V and z, each against the
    reference and against each other at the bound."""
    a, _, _ = run(X, d, k, prec, 1)
    b, _, _ = run(X, d, k, prec, 0, lead=1)
    bound = C.reference(d, k, prec)[3]
    r = float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / bound).max())
    print(f"MEASURED paths 1 - 0 {prec} d = {d} k = {k}: difference / bound {r:.3g}")
    assert r <= 1.0


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("d,k", C.BATCHED, ids=lambda v: str(v))
def test_batched_sweeps(d, k, prec):
    if (d, k) in C.CHUNK_CASES:
        assert C.rd_chunks(d, k) == C.CHUNK_CASES[(d, k)]
    X = handle(d, prec)
    try:
        if d % C.E[prec] == 0:      # d = 32, 64: whole 16-byte vectors, the batched path needs the misaligned z
            both_paths(X, d, k, prec)
        else:
            run(X, d, k, prec, 0)
    finally:
        X.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("nv,k", C.PIECE, ids=lambda v: str(v))
def test_piece_sweeps(nv, k, prec):
    d = nv * C.E[prec]
    if k == C.PIECE_CHUNKS_K and nv in C.PIECE_CHUNKS_NV:
        assert C.rdv_steps_chunks(nv) == C.PIECE_CHUNKS_NV[nv]
    X = handle(d, prec)
    try:
        both_paths(X, d, k, prec)
    finally:
        X.close()


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_state_flag_of_a_broken_down_recurrence_is_cleared(prec):
    """A recurrence that broke down leaves the device flag set, and every CGS2 kernel returns early on it: a
    krcn_cgs2 call after it must still sweep (d = 25: batched; d = 24: the 1 KiB pieces)."""
    for d, path in ((25, 0), (24, 1)):
        A, b = synth.make_problem(None, seed=7, n=200, d=d, nnz=3000)
        X = krcn.DeviceCSR(A, dtype=TORCH[prec])
        try:
            Ax = X.matvec(torch.full((d,), 0.5, dtype=TORCH[prec], device=DEV))
            g = X.gradient(Ax, torch.from_numpy(O.labels01(b)).to(DEV, TORCH[prec]))
            _, _, _, info = X.lanczos(X.weights(Ax), g, 40, reorth=True)
            assert info.breakdown == 1
            run(X, d, 5, prec, path)
        finally:
            X.close()


def test_errors_that_need_a_handle():
    X = handle(33, "fp64")
    try:
        lib = _lib.load()
        z = torch.zeros(33, dtype=torch.float64, device=DEV)
        V = torch.zeros((3, 33), dtype=torch.float64, device=DEV)
        for Vp, zp in ((None, z.data_ptr()), (V.data_ptr(), None)):
            assert lib.krcn_cgs2(X.handle, 3, Vp, zp, None, None, None) == _lib.KRCN_ERR_INVALID
            assert b"krcn_cgs2: null argument" in lib.krcn_last_error_string()
        assert lib.krcn_cgs2(X.handle, 2044, V.data_ptr(), z.data_ptr(), None, None, None) == _lib.KRCN_ERR_INVALID
        # both out pointers may be NULL
        torch.cuda.synchronize()
        assert lib.krcn_cgs2(X.handle, 3, V.data_ptr(), z.data_ptr(), None, None, None) == _lib.KRCN_OK
        with pytest.raises(ValueError):
            X.cgs2(V, z, k=4)
    finally:
        X.close()


# ------------------------------------------------ through krcn_lanczos(reorth=True)
def test_recurrence_odd_d_crosses_the_cache_boundary_and_chunk_counts():
    """d = 8193 (odd: the batched sweeps), m = 300, fp64: the recurrence's own sweeps go from C = 2 chunks to 1 at
    k = 513 > m (so C = 2 from k = 1: cgs_rd_chunks(8193, k) = min(1024 // k, 2)) and from the cached to the
    uncached update at k = 257, on buffers sized by reserve_reorth.  Against the oracle's CGS2 at the tolerances
    of tests/test_gpu_lanczos.py (1e-10; basis orthonormal to 1e-12).  The matrix has two nonzeros a row: on
    denser ones of this shape the oracle's own alphas move by 1e-2 under a 1e-16 perturbation of the HVP at
    m = 300 (here: 1e-14)."""
    A, b = synth.make_problem(None, seed=31, n=6000, d=8193, nnz=12_000)
    x = np.full(A.shape[1], 0.5)
    X = krcn.DeviceCSR(A)
    try:
        Ax = X.matvec(torch.from_numpy(x).to(DEV))
        w = X.weights(Ax)
        g = X.gradient(Ax, torch.from_numpy(O.labels01(b)).to(DEV))
        m = 300
        assert X.lanczos_step(reorth=True) == "generic"
        V, al, be, info = X.lanczos(w, g, m, reorth=True)
        assert info.m_eff == m
        wh = O.hessian_weights(A, x)
        _, al_r, be_r, _ = O.lanczos_cgs2(lambda v: O.hvp_from_weights(A, wh, v), g.cpu().numpy(), m)
        print(f"MEASURED recurrence d = 8193 m = 300: alphas {rel_err(al, al_r):.3g}, betas {rel_err(be, be_r):.3g}")
        assert rel_err(al, al_r) < 1e-10
        assert rel_err(be, be_r) < 1e-10
        Vh = V.cpu().numpy()
        assert np.abs(Vh @ Vh.T - np.eye(m)).max() < 1e-12
    finally:
        X.close()


def test_recurrence_column_sharded_on_two_virtual_ranks():
    """reorth=True on column shards (reorth_cgs2's over_ranks branch: the chunk partials summed per rank by
    k_cgs_coeffs, all-reduced, and handed to the update as one chunk; h2 all-reduced before the norm sweep), two
    virtual ranks, m = 40, d = 101: alphas / betas against the oracle's CGS2 at 1e-10 on every rank, bitwise
    equal across ranks, the rank blocks of V side by side orthonormal to 1e-12.  krcn_cgs2 itself refuses a
    sharded handle."""
    A, b = synth.make_problem(None, seed=7, n=400, d=101, nnz=6000)
    m = 40
    vs = kdist.VirtualShards(A, b, 2, partition="cols")
    try:
        assert vs.mode == "cols"

        def fn(r):
            X = vs.X[r]
            X.reserve(m, reorth=True)     # collective-free calls below: the workspace exists before the recurrence
            x = torch.full((X.d,), 0.5, dtype=X.dtype, device=X.device)
            Ax = X.matvec(x)
            g = X.gradient(Ax, vs.b[r])
            V, al, be, info = X.lanczos(X.weights(Ax), g, m, reorth=True)
            z = torch.zeros(X.d, dtype=X.dtype, device=X.device)
            st = _lib.load().krcn_cgs2(X.handle, 3, V.data_ptr(), z.data_ptr(), None, None, None)
            return V.cpu().numpy(), al, be, info.m_eff, g.cpu().numpy(), st

        res = vs.run(fn)
    finally:
        vs.close()
    x = np.full(A.shape[1], 0.5)
    wh = O.hessian_weights(A, x)
    gh = O.gradient(A, O.labels01(b), x)
    assert rel_err(np.concatenate([r[4] for r in res]), gh) < 1e-13
    _, al_r, be_r, _ = O.lanczos_cgs2(lambda v: O.hvp_from_weights(A, wh, v), gh, m)
    for _, al, be, m_eff, _, st in res:
        assert m_eff == m == len(al_r)
        assert rel_err(al, al_r) < 1e-10
        assert rel_err(be, be_r) < 1e-10
        np.testing.assert_array_equal(al, res[0][1])
        np.testing.assert_array_equal(be, res[0][2])
        assert st == _lib.KRCN_ERR_UNSUPPORTED
    print(f"MEASURED recurrence cols x 2: alphas {rel_err(res[0][1], al_r):.3g}, betas {rel_err(res[0][2], be_r):.3g}")
    Vh = np.concatenate([r[0] for r in res], axis=1)
    assert Vh.shape == (m, A.shape[1])
    assert np.abs(Vh @ Vh.T - np.eye(m)).max() < 1e-12
