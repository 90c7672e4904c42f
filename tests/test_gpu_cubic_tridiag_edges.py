"""krcn_cubic_tridiag (csrc/krcn_cubic.hpp) at the sizes where its loops change
shape, element by element.

krcn_cubic_tridiag_block and the solver inside krcn_crn_step /
krcn_crn_step_block are compared with this call bitwise
(tests/test_gpu_crn_step_block.py), so whatever it gets wrong they reproduce.
Elsewhere it runs at m in {1, 2, 3, 10, 50} only (tests/test_gpu_crn_step.py):
m % 8 in {1, 2, 3}, one trip of every `for (i = tid; i < m; i += kNT)`.

The serial sweeps walk LDS in chunks of kCubicChunk = 8 with a scalar tail each:
  cubic_factor    chunks while i + 8 < m from i = 0, tail while i + 1 < m;
  cubic_forward   chunks while i + 8 <= m from i = 1, tail while i < m;
  cubic_backward  chunks while i - 7 >= 0 from i = m - 2, tail down to 0.
m = 7, 8, 9 (and 15..17, 63..65) put an empty tail, a one-element tail and no
chunk at all on each of them; 255..257, 511, 513, 1023, 1025 the second to
fifth trips of the all-thread loops (kNT = 256); 2043 and 2044 the end of the
six 2044-entry LDS arrays, 2045 the refusal above it.

References: optimizer.cubic.cubic_solver_root_tridiag (LAPACK dpttrf / dpttrs:
the same sweeps in the same order) and, independent of it, the oracle's dense
cubic_solver_root on T.  Bounds: 1e-13 with equal Newton iteration counts (the
bound of test_gpu_crn_step.py's check_subproblem); element-wise on the slowly
decaying matrices max(1e-13, 10 x the element-wise spread between the two host
references on that case), computed here; 1e-10 on the step (that file's fp64
bound).  What each test would catch is in its docstring, argued from the code.
"""
import ctypes
import functools
import warnings

import numpy as np
import numpy.linalg as la
import pytest

import krcn
import krcn_oracle as O
from conftest import rel_err
from krcn import _lib, synth
from optimizer import cubic as C
from test_gpu_crn_step import assert_same_decisions, make_opt

gpu = pytest.mark.gpu

G0, R0, EPS = 0.3, 0.1, 1e-8
EDGE_M = [7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025, 2043, 2044]
EDGE_REG = [1e-3, 2.0]
TAIL_M = [257, 1025, 2044]
TAIL_REG = [1e-6, 1e-3]
SOLVER_FIELDS = ("solver_it", "solver_status", "reg_coef", "lam", "model_decrease")
POISON_CALLS = 16    # two launches per call: four rounds over the eight dies that take workgroups in turn


def _draw_edges():
    rng = np.random.default_rng(5)
    out = {}
    for m in EDGE_M:                                   # drawn in this order from one generator
        out[m] = (rng.uniform(0.5, 1.5, m), rng.uniform(-0.2, 0.2, m - 1))
    return out


def _draw_tails():
    rng = np.random.default_rng(5)
    return {m: (2.0 + 1e-4 * (1.0 + rng.uniform(0.0, 1.0, m)), np.full(m - 1, -1.0)) for m in TAIL_M}


EDGES, TAILS = _draw_edges(), _draw_tails()
for _al, _be in list(EDGES.values()) + list(TAILS.values()):
    _al.setflags(write=False), _be.setflags(write=False)


def e1(m):
    g = np.zeros(m)
    g[0] = G0
    return g


@functools.lru_cache(maxsize=None)
def host_edge(m, M):
    """The host solver on an item-a matrix: (s, its, lam, dec), read-only."""
    out = C.cubic_solver_root_tridiag(e1(m), *EDGES[m], M, epsilon=EPS, r0=R0)
    out[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_tail(m, M):
    """Both host references on a slowly decaying matrix: the tridiagonal solver's
    (s, its, lam, dec) and the dense oracle's on T."""
    al, be = TAILS[m]
    tri = C.cubic_solver_root_tridiag(e1(m), al, be, M, epsilon=EPS, r0=R0)
    T = np.diag(al) + np.diag(be, 1) + np.diag(be, -1)
    dense = O.cubic_solver_root(e1(m), T, M, epsilon=EPS, r0=R0)
    tri[0].setflags(write=False), dense[0].setflags(write=False)
    return tri, dense


@pytest.fixture(scope="module")
def handle():
    A, _ = synth.make_problem(None, seed=5, n=64, d=16, nnz=256)
    X = krcn.DeviceCSR(A)
    yield X
    X.close()


# ---------------------------------------------------- chunk and stride edges
@gpu
@pytest.mark.parametrize("m", EDGE_M)
def test_chunk_and_stride_edges(handle, m):
    """alphas ~ U(0.5, 1.5), betas ~ U(-0.2, 0.2), g = 0.3 e1, M in {1e-3, 2}
    against the host solver: status 0, equal Newton counts, s (max-norm), lam
    and the model decrease within 1e-13.  Each m is preceded by POISON_CALLS
    solves of m + 1 entries whose last alpha is -5: status 1 from the last
    pivot alone, which also leaves a negative pivot in dd[m] and a multiplier
    in ee[m - 1], the LDS entries just past what a solve of m entries
    initialises.  LDS is not cleared between launches, and successive
    one-workgroup launches go to the dies in turn, hence the repetition;
    nothing promises that a later launch finds those values.

    Would catch: `i + C <= m` in cubic_factor (at m = 8, 16, 64, 256 the last
    chunk forms one pivot too many, from e[m - 1] and d[m]: with the negative
    pivot left there the factorisation reports status 1.  A build with that
    change failed at m = 8, 16, 64 and 256 and nowhere else; with a single
    preceding solve it passed all four, and with none it failed at 64 and 256
    on whatever LDS held); a factor loop that stops one pivot early or drops
    its closing `return di > 0` (the solve of m + 1 entries reports status 0); a
    forward sweep whose tail starts one entry late or a chunk that stores one
    place off at m = 7..17, where the entries involved still carry weight (a
    build whose backward tail starts at m - 3 failed here at m = 7, 8 and 9
    only).  s decays by a factor of about |beta| / alpha per entry, so
    anything that only changes s, y or z past the first few dozen entries is
    invisible to this max-norm and to lam: that is test_tail_of_s's part (a
    build with `y[i] / dd[i]` applied to the first kNT entries only failed
    every case there and none here).

    Measured on an MI355X: s within 1.9e-17 of the host solver's largest entry
    (bitwise equal in 34 of the 36 cases), lam within 1.8e-16 and the model
    decrease within 1.3e-16; counts equal."""
    al, be = EDGES[m]
    if m < EDGE_M[-1]:
        for _ in range(POISON_CALLS):
            sp, ip = handle.cubic_tridiag(np.append(al, -5.0), np.append(be, 0.1), G0, 1e-3, r0=R0, eps=EPS)
            assert ip.solver_status == 1 and not sp.any()
    for M in EDGE_REG:
        s_ref, its, lam, dec = host_edge(m, M)
        s, info = handle.cubic_tridiag(al, be, G0, M, r0=R0, eps=EPS)
        es, el, ed = rel_err(s, s_ref), abs(info.lam - lam) / abs(lam), abs(info.model_decrease - dec) / abs(dec)
        print(f"m = {m} M = {M:g}: {info.solver_it} iterations, s {es:.2e}, lam {el:.2e}, decrease {ed:.2e}")
        assert info.solver_status == 0
        assert info.solver_it == its
        assert np.abs(s - s_ref).max() <= 1e-13 * np.abs(s_ref).max()
        assert el <= 1e-13
        assert ed <= 1e-13
        assert info.reg_coef == M


# ------------------------------------------------------------ the tail of s
@pytest.mark.parametrize("M", TAIL_REG)
@pytest.mark.parametrize("m", TAIL_M)
def test_tail_matrices_keep_s_representable(m, M):
    """CPU, on the host reference alone: with alphas = 2 + 1e-4 (1 + U(0, 1)) and
    betas = -1 the solution decays so slowly that its last entry is still a
    normal number far above the underflow of the comparison below, and the two
    host references agree on the iteration count."""
    (s, its, lam, dec), (sd, itsd, lamd, decd) = host_tail(m, M)
    ratio = np.abs(s).min() / np.abs(s).max()
    spread = (np.abs(s - sd) / np.abs(s)).max()
    print(f"m = {m} M = {M:g}: min|s| / max|s| = {ratio:.2e}, {its} iterations, element-wise spread of the "
          f"host references {spread:.2e}")
    assert ratio >= 1e-40
    assert its == itsd
    # test_tail_of_s allows ten times this spread: it has to stay many orders below the order-one
    # errors that test exists to see (dpttrs against a dense Cholesky at cond ~ 1e4: about 1e-12)
    assert spread < 1e-10


@gpu
@pytest.mark.parametrize("M", TAIL_REG)
@pytest.mark.parametrize("m", TAIL_M)
def test_tail_of_s(handle, m, M):
    """Every entry of s against the host solver, relative to that entry, on
    matrices whose solution stays representable to the last one.

    Would catch: a backward tail starting at m - 3 (s[m - 2] keeps q[m - 2]
    without its - s[m - 1] e[m - 2] term: an order-one error there that the
    max-norm of a decaying s cannot see), a backward chunk loop with
    `i - (C - 1) > 0` (harmless) or `i - C >= 0` with the tail unchanged
    (harmless); a forward chunk that stores bv[k] one place off; a division
    or store loop that stops at kNT (s[256..] undivided or zero: every one of
    them fails).  Builds with the first and with the last-but-one of these
    changes failed all six cases.

    tol = max(1e-13, 10 x the element-wise spread between the tridiagonal host
    solver and the dense oracle on T): the device runs the host's recurrences
    and differs only in the order of the dot sums.
    Measured on an MI355X: every entry of s equals the host solver's bitwise on
    all six cases (the host references are 2.0e-14 to 2.7e-13 apart, so tol is
    2.0e-13 to 2.7e-12); counts equal (19 at M = 1e-6, 10 at M = 1e-3)."""
    al, be = TAILS[m]
    (s_ref, its, lam, dec), (s_dense, _, _, _) = host_tail(m, M)
    spread = (np.abs(s_ref - s_dense) / np.abs(s_ref)).max()
    tol = max(1e-13, 10 * spread)
    s, info = handle.cubic_tridiag(al, be, G0, M, r0=R0, eps=EPS)
    err = (np.abs(s - s_ref) / np.abs(s_ref)).max()
    print(f"m = {m} M = {M:g}: element-wise {err:.2e} (tol {tol:.2e}, host spread {spread:.2e}), "
          f"{info.solver_it} iterations")
    assert info.solver_status == 0
    assert info.solver_it == its
    assert (np.abs(s - s_ref) <= tol * np.abs(s_ref)).all()


# --------------------------------------------------------- statuses at size
@gpu
@pytest.mark.parametrize("m", [257, 2044])
def test_it_max_returns_the_last_iterate_at_size(handle, m):
    """it_max = 2 on a case that needs more: status 3 with the host's second
    iterate (root_scalar returns it without raising), s from the closing solve
    at that lam.  Would catch a closing solve skipped on kCubicItMax (s zero)
    at sizes where the store loop takes more than one trip."""
    al, be = EDGES[m]
    M = 1e-3
    assert host_edge(m, M)[1] > 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s_ref, its, lam, dec = C.cubic_solver_root_tridiag(e1(m), al, be, M, it_max=2, epsilon=EPS, r0=R0)
    s, info = handle.cubic_tridiag(al, be, G0, M, r0=R0, eps=EPS, it_max=2)
    assert info.solver_status == 3 and info.solver_it == its == 2
    assert abs(info.lam - lam) <= 1e-13 * abs(lam)
    assert abs(info.model_decrease - dec) <= 1e-13 * abs(dec)
    assert np.abs(s - s_ref).max() <= 1e-13 * np.abs(s_ref).max()


@gpu
@pytest.mark.parametrize("m", [8, 9, 257, 2044])
def test_indefinite_last_pivot_is_a_status(handle, m):
    """alpha[m - 1] = -5 with |beta| <= 0.2 leaves T + r0 I indefinite, and only
    the last pivot shows it: the host raises from dpttrf, the device reports
    status 1 and s = 0.  The last pivot is formed by the last step of the
    scalar tail (m = 8, 257, 2044) or of the last chunk (m = 9) and is tested
    by cubic_factor's closing `return di > 0`.  Would catch a factor loop that
    stops one pivot early (`i + 2 < m`), or a closing test dropped."""
    al, be = EDGES[m]
    al = al.copy()
    al[-1] = -5.0
    with pytest.raises(la.LinAlgError):
        C.cubic_solver_root_tridiag(e1(m), al, be, 1e-3, epsilon=EPS, r0=R0)
    s, info = handle.cubic_tridiag(al, be, G0, 1e-3, r0=R0, eps=EPS)
    assert info.solver_status == 1
    assert len(s) == m and not s.any()


@gpu
def test_m_above_the_lds_arrays_is_refused(handle):
    """m = 2045 is one more than the LDS arrays hold: KRCN_ERR_INVALID before
    anything is touched (s and info keep what the caller put there), and the
    handle goes on working."""
    from krcn.device import _stream
    m = 2045
    al, be = np.ones(m), np.full(m - 1, 0.1)
    s = np.full(m, -7.0)
    info = _lib.CrnInfo()
    info.solver_it, info.lam = 41, -3.0
    with pytest.raises(_lib.KrcnError) as e:
        _lib.call("krcn_cubic_tridiag", handle.handle, m, al.ctypes.data_as(_lib._dp), be.ctypes.data_as(_lib._dp),
                  G0, 1e-3, R0, EPS, 100, s.ctypes.data_as(_lib._dp), ctypes.byref(info), _stream(handle.device))
    assert e.value.status == _lib.KRCN_ERR_INVALID
    assert (s == -7.0).all() and info.solver_it == 41 and info.lam == -3.0
    with pytest.raises(_lib.KrcnError) as e:
        handle.cubic_tridiag(al, be, G0, 1e-3)
    assert e.value.status == _lib.KRCN_ERR_INVALID
    s8, i8 = handle.cubic_tridiag(*EDGES[8], G0, 1e-3, r0=R0, eps=EPS)
    assert i8.solver_status == 0 and np.abs(s8 - host_edge(8, 1e-3)[0]).max() <= 1e-13 * np.abs(s8).max()


# ------------------------------------------- the block solver at mixed sizes
@gpu
def test_block_solver_at_mixed_sizes_is_bitwise_the_single_call(handle):
    """One krcn_cubic_tridiag_block call with columns of m_eff = 1, 8, 9, 257 and
    2044 (row stride 2044): each column's s and solver fields are bitwise the
    single call's.  Would catch a column reading its alphas / betas at the
    stride of its own m_eff, a workgroup leaving LDS of a longer column's sweep
    to a shorter one's tail, or the rows of s past m_eff not zeroed."""
    cols = [(np.array([0.7]), np.array([]), 1e-3), (*EDGES[8], 2.0), (*EDGES[9], 1e-3), (*TAILS[257], 1e-6),
            (*EDGES[2044], 2.0)]
    al, be, Ms = [c[0] for c in cols], [c[1] for c in cols], [c[2] for c in cols]
    s, infos = handle.cubic_tridiag_block(al, be, G0, Ms, r0=R0, eps=EPS)
    for c in range(len(cols)):
        s1, i1 = handle.cubic_tridiag(al[c], be[c], G0, Ms[c], r0=R0, eps=EPS)
        assert i1.solver_status == 0
        assert s[c].tobytes() == s1.tobytes(), c
        for f in SOLVER_FIELDS:
            assert getattr(infos[c], f) == getattr(i1, f), (c, f)


# ------------------------------------------- the step at m past one block
@gpu
def test_step_with_m_past_one_block():
    """One Krylov-CRN step at m = 264 > kNT from x = 0.5: the device step against
    the host path, which runs the same device Lanczos and the host subproblem.
    Equal trials, accept decisions and Newton counts; x and f within 1e-10.
    Runs k_crn_begin's copy loops (`lz[4 + i]`, `lz[4 + m + i]`) and the solver
    inside the chain on their second trip; would catch a copy that stops at
    kNT (alphas[256..] and betas[256..] are then whatever the workspace held).
    Measured on an MI355X: m_eff = 264, x and f bitwise equal, 8 Newton
    iterations on both paths."""
    A, b = synth.make_problem(None, seed=8, n=900, d=320, nnz=18_000)
    opts = []
    for device_step in (False, True):
        opt = make_opt(A, b, device_step, m=264)
        opt.run(x0=np.full(A.shape[1], 0.5), it_max=1)
        opts.append(opt)
    host, dev = opts
    assert dev.last_lanczos.m_eff > 256
    assert_same_decisions(host, dev)
    ex = rel_err(dev.x.cpu().numpy(), host.x.cpu().numpy())
    ev = abs(dev.value - host.value) / abs(host.value)
    print(f"m = 264 (m_eff {dev.last_lanczos.m_eff}): x rel {ex:.2e}, f rel {ev:.2e}, solver_it {dev.solver_it}")
    assert ex < 1e-10
    assert ev <= 1e-10
