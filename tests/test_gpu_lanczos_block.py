"""Batched Lanczos (krcn_lanczos_block): k recurrences of cubic.py:77-111 in
lockstep over the block HVP, with krcn_basis_combine_block / krcn_weights_block.

Expectations come from oracle/krcn_oracle.py's `lanczos` over `hvp_from_weights`
(pinned bitwise to the reference) on f1's operator (257 x 513):
  * the gradient column reproduces f2["alphas_m10"] exactly; its smallest beta
    is 1.6e-3;
  * weights that are zero except on the r longest rows (5, 100, 200), started
    from default_rng(7).standard_normal(d), break down at loop index j = r, for
    r = 1 and r = 3, at l2 = 0 and l2 = 0.01; the breaking beta is 7e-18 .. 5e-15
    and the last surviving one >= 5e-4, decades from the 1e-6 threshold on both
    sides (test_cases_are_what_they_claim checks all of this on the CPU);
  * m = r + 2 keeps the zero last vector, m >= r + 3 truncates to r + 1.
A 2e-16 relative perturbation of the oracle's HVP moves alpha by <= 1.3e-14,
beta by <= 7e-16 and V by <= 1.2e-8 at m = 10, so the suite's Lanczos bounds
apply: alphas / betas rel_err < 1e-11, V of columns that do not break max-abs
1e-6 (test_gpu_lanczos.py::test_lanczos_vs_golden), and for breaking columns
the exact structure plus the three-term residual < 1e-12 hn of
test_lanczos_three_term_relation instead of a V bound.

Grid cap: the vector kernels run on at most 1024 workgroups (kBlzMaxGrid), each
covering 4 * 256 / K rows a round, K the next power of two >= k: 65,536 rows a
grid stride at K = 16.  test_more_than_one_grid_stride crosses it.
"""
import numpy as np
import pytest
import torch

import krcn
import krcn_oracle as O
from conftest import golden_csr, rel_err
from krcn import _lib
from optimizer.loss import LogisticRegression
from test_gpu_block import POS_A, edge_matrix, long_matrix

gpu = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-6
MS = (1, 2, 3, 5, 6, 10)
PARTIALS_BYTES = 3 * 1024 * 16 * 8


def t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def h(x):
    return x.detach().cpu().numpy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def oracle_column(A, w, g, m, l2):
    """The oracle's outcome for one column, with the info fields krcn_lanczos reports."""
    V, al, be, beta = O.lanczos(lambda v: O.hvp_from_weights(A, w, v, l2), g, m)
    broke = m > 1 and abs(beta) < TOL
    m_eff = V.shape[1]
    j_break = -1 if not broke else (m_eff - 1 if m_eff < m else m - 2)
    return dict(V=V, al=al, be=be, beta=float(beta), m_eff=m_eff, breakdown=int(broke), j_break=j_break,
                hvps=(j_break + 1 if broke else m - 1) + 1, gnorm=float(np.linalg.norm(g)))


class Problem:
    """f1's operator and the five columns of the mixed batch."""

    def __init__(self, f1, f2):
        self.A = A = golden_csr(f1)
        self.n, self.d = A.shape
        self.w = O.hessian_weights(A, f1["x0"])
        self.g = np.array(f2["g"])
        self.s = np.random.default_rng(7).standard_normal(self.d)
        longest = np.argsort(-np.diff(A.indptr), kind="stable")
        self.longest = longest[:3]

        def rank(r):
            wr = np.zeros(self.n)
            wr[longest[:r]] = self.w[longest[:r]]
            return wr

        self.rank = rank
        # (weights, start, l2, rank or None)
        self.cols = [(self.w, self.g, 0.0, None), (self.w, self.s, 0.01, None), (rank(1), self.s, 0.0, 1),
                     (rank(3), self.s, 0.0, 3), (rank(3), self.s, 0.01, 3)]
        self._ref = {}

    def batch(self, cols=None):
        cols = self.cols if cols is None else cols
        W = np.stack([c[0] for c in cols], axis=1)
        G = np.stack([c[1] for c in cols], axis=1)
        return W, G, np.array([c[2] for c in cols])

    def ref(self, c, m):
        if (c, m) not in self._ref:
            w, g, l2, _ = self.cols[c]
            self._ref[(c, m)] = oracle_column(self.A, w, g, m, l2)
        return self._ref[(c, m)]


@pytest.fixture(scope="module")
def prob(f1, f2):
    return Problem(f1, f2)


@pytest.fixture(scope="module")
def X(prob):
    return krcn.DeviceCSR(prob.A)


@pytest.fixture(scope="module")
def mixed(prob, X):
    """One lanczos_block call per m of the mixed batch, from a NaN-filled V."""
    W, G, l2 = prob.batch()
    out = {}
    for m in MS:
        V = torch.full((m, prob.d, 5), float("nan"), dtype=torch.float64, device=DEV)
        Vd, al, be, infos = X.lanczos_block(t(W), t(G), m, l2=l2, V=V)
        out[m] = (h(Vd), al, be, infos)
    return out


def check_column(got_al, got_be, info, Vc, ref, m, A, w, l2, where):
    """One column against its oracle: structure exactly, alphas / betas at 1e-11, then V
    (max-abs 1e-6) when it does not break, the three-term residual when it does."""
    assert (info.m_eff, info.breakdown, info.j_break, info.hvps) == \
        (ref["m_eff"], ref["breakdown"], ref["j_break"], ref["hvps"]), where
    assert got_al.shape == ref["al"].shape and got_be.shape == ref["be"].shape, where
    e_al, e_be = rel_err(got_al, ref["al"]), rel_err(got_be, ref["be"])
    print(f"{where}: alphas {e_al:.2e} betas {e_be:.2e} beta_last {info.beta_last:.2e}")
    assert e_al < 1e-11 and e_be < 1e-11, where
    assert (info.beta_last < TOL) == (ref["beta"] < TOL), where
    assert abs(info.gnorm - ref["gnorm"]) <= 1e-13 * ref["gnorm"], where
    me = info.m_eff
    cur = info.j_break if info.breakdown else m - 1
    # every slab that holds no basis vector of the column is byte-zero (the zero last vector included)
    assert not Vc[cur + 1:].view(np.uint8).any(), where
    if not info.breakdown:
        assert abs(info.beta_last - ref["beta"]) <= 1e-11 * abs(ref["beta"]), where
        assert np.abs(Vc[:me].T - ref["V"]).max() < 1e-6, where
        return
    if info.j_break == m - 2:
        assert me == m and got_be[-1] == 0.0, where
    H = lambda v: O.hvp_from_weights(A, w, v, l2)  # noqa: E731
    hn = max(np.abs(got_al).max(), np.abs(got_be).max() if got_be.size else 0.0)
    for j in range(me - 1):
        r = H(Vc[j]) - got_al[j] * Vc[j] - got_be[j] * Vc[j + 1] - (got_be[j - 1] * Vc[j - 1] if j else 0)
        assert np.linalg.norm(r) < 1e-12 * hn, (where, j)
    assert abs(got_al[-1] - Vc[cur] @ H(Vc[cur])) < 1e-12 * hn, where


# ------------------------------------------------------------- CPU: the cases
def test_cases_are_what_they_claim(prob, f2):
    assert tuple(prob.longest) == (5, 100, 200)
    for m in (1, 10):
        assert np.array_equal(prob.ref(0, m)["al"], f2[f"alphas_m{m}"])
    assert prob.ref(0, 10)["be"].min() > 1.5e-3
    for c, (_, _, _, r) in enumerate(prob.cols):
        for m in MS:
            ref = prob.ref(c, m)
            if r is None or m < r + 2:
                assert not ref["breakdown"] and ref["m_eff"] == m
            else:
                assert ref["breakdown"] and ref["j_break"] == r and ref["beta"] < 1e-14
                assert ref["m_eff"] == (m if m == r + 2 else r + 1)
            kept = ref["be"][ref["be"] != 0]   # (a break at j == m - 2 leaves betas[m - 2] = 0)
            assert kept.size == ref["m_eff"] - 1 - (1 if ref["breakdown"] and ref["j_break"] == m - 2 else 0)
            assert kept.size == 0 or kept.min() >= 5e-4


# ----------------------------------------------------------- 1. golden column
@gpu
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("m", [1, 10])
def test_golden_column(prob, X, f2, k, m):
    cols = [prob.cols[0], prob.cols[1], prob.cols[3]][:k]
    W, G, l2 = prob.batch(cols)
    V, al, be, infos = X.lanczos_block(t(W), t(G), m, l2=l2)
    info = infos[0]
    assert info.m_eff == m and not info.breakdown and info.hvps == m and info.j_break == -1
    assert rel_err(al[0], f2[f"alphas_m{m}"]) < 1e-11
    assert rel_err(be[0], f2[f"betas_m{m}"]) < 1e-11
    assert np.abs(h(V)[:, :, 0].T - f2[f"V_m{m}"]).max() < 1e-6
    assert abs(info.beta_last - float(f2[f"beta_m{m}"])) <= 1e-11 * max(1e-300, abs(float(f2[f"beta_m{m}"])))
    assert abs(info.gnorm - np.linalg.norm(f2["g"])) <= 1e-13 * np.linalg.norm(f2["g"])


# -------------------------------------------------------------- 2. mixed batch
@gpu
@pytest.mark.parametrize("m", MS)
def test_mixed_batch_vs_oracle(prob, mixed, m):
    V, al, be, infos = mixed[m]
    assert V.shape == (m, prob.d, 5)
    for c, (w, _, l2, _) in enumerate(prob.cols):
        check_column(al[c], be[c], infos[c], np.ascontiguousarray(V[:, :, c]), prob.ref(c, m), m, prob.A, w, l2,
                     f"m {m} column {c}")


# ------------------------------------------- 3. agreement with the single call
@gpu
@pytest.mark.parametrize("m", MS)
def test_columns_agree_with_the_single_call(prob, X, mixed, m):
    _, al, be, infos = mixed[m]
    for c, (w, g, l2, _) in enumerate(prob.cols):
        _, sal, sbe, si = X.lanczos(t(w), t(g), m, l2=l2)
        bi = infos[c]
        assert (bi.m_eff, bi.breakdown, bi.j_break, bi.hvps) == (si.m_eff, si.breakdown, si.j_break, si.hvps)
        assert al[c].shape == sal.shape and be[c].shape == sbe.shape
        assert rel_err(al[c], sal) < 1e-11 and rel_err(be[c], sbe) < 1e-11
        assert (bi.beta_last < TOL) == (si.beta_last < TOL)
        assert abs(bi.gnorm - si.gnorm) <= 1e-13 * si.gnorm


# ---------------------------------------------------- 4. column independence
@gpu
@pytest.mark.parametrize("m", [3, 6])
def test_column_independence_and_run_to_run(prob, X, m):
    rng = np.random.default_rng(11)
    a = prob.cols
    other = [(prob.rank(1), rng.standard_normal(prob.d), 0.01, 1), (prob.w, rng.standard_normal(prob.d), 0.0, None),
             (prob.rank(3), prob.g, 0.0, 3)]
    b = [a[0], other[0], other[1], a[3], other[2]]
    runs = []
    for cols in (a, b, a):
        W, G, l2 = prob.batch(cols)
        V, al, be, infos = X.lanczos_block(t(W), t(G), m, l2=l2)
        runs.append((h(V), al, be))
    (Va, ala, bea), (Vb, alb, beb), (Va2, ala2, bea2) = runs
    for c in (0, 3):
        assert same_bytes(ala[c], alb[c]) and same_bytes(bea[c], beb[c])
        assert same_bytes(Va[:, :, c], Vb[:, :, c])
    assert not same_bytes(Va[:, :, 1], Vb[:, :, 1])
    assert same_bytes(Va, Va2)
    for c in range(5):
        assert same_bytes(ala[c], ala2[c]) and same_bytes(bea[c], bea2[c])


# ------------------------------------------- 5. grid and lane-group edges
def edge_case(A, k, seed):
    n, d = A.shape
    rng = np.random.default_rng(seed + 100 * k)
    return rng.uniform(0.05, 0.25, n), rng.standard_normal((d, k))


def check_shared_weights(A, Xd, k, m, seed, where):
    w, G = edge_case(A, k, seed)
    V, al, be, infos = Xd.lanczos_block(t(w), t(G), m)
    Vh = h(V)
    for c in range(k):
        ref = oracle_column(A, w, G[:, c], m, 0.0)
        assert all(b_ == 0 or b_ > 1e-5 for b_ in ref["be"])   # nothing near the threshold decides a case
        assert ref["beta"] == 0 or ref["beta"] > 1e-5 or ref["beta"] < 1e-9
        check_column(al[c], be[c], infos[c], np.ascontiguousarray(Vh[:, :, c]), ref, m, A, w, 0.0,
                     f"{where} k {k} column {c}")
    return infos


@gpu
@pytest.mark.parametrize("d", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025])
def test_grid_and_lane_group_edges(d):
    A = edge_matrix(40, d, seed=d)
    Xd = krcn.DeviceCSR(A)
    for k in (1, 2, 3, 5, 8, 13, 16):
        infos = check_shared_weights(A, Xd, k, 3, d, f"d {d}")
        if d == 1:
            assert all(i.breakdown and i.j_break == 0 and i.m_eff == 1 for i in infos)
        if d == 2:
            assert all(i.breakdown and i.j_break == 1 and i.m_eff == 3 for i in infos)


@gpu
def test_more_than_one_grid_stride():
    """K = 16: 1024 workgroups x 64 rows = 65,536 rows a stride (the cap: kBlzMaxGrid = 1024)."""
    d = 65536 + 37
    A = edge_matrix(40, d, seed=3)
    check_shared_weights(A, krcn.DeviceCSR(A), 16, 3, 3, "grid stride")


@gpu
def test_long_rows():
    A = long_matrix(list(POS_A), 1)
    assert np.diff(A.indptr).max() > _lib.KRCN_BLOCK_LONG_ROW
    check_shared_weights(A, krcn.DeviceCSR(A), 8, 3, 1, "long rows")


# ------------------------------------------------- 6. smaller entry points
@gpu
@pytest.mark.parametrize("k", [1, 3, 8])
def test_basis_combine_block(prob, X, k):
    m, d = 19, prob.d
    rng = np.random.default_rng(5 + k)
    V = rng.standard_normal((m, d, k))
    S = rng.standard_normal((m, k))
    for c in range(k):
        S[3 + c:, c] = 0.0          # zero-padded past each column's "m_eff"
    X0 = rng.standard_normal((d, k))
    got = h(X.basis_combine_block(t(V), S, t(X0)))
    acc = np.zeros((d, k))
    for j in range(m):
        acc = acc + V[j] * S[j]
    assert rel_err(got, X0 + acc) < 1e-14
    for c in range(k):
        single = h(X.basis_combine(t(V[:, :, c]), S[:, c], t(X0[:, c])))
        assert same_bytes(got[:, c], single)


@gpu
def test_weights_block(prob, X):
    rng = np.random.default_rng(9)
    k, n = 5, prob.n
    AX = 3.0 * rng.standard_normal((n, k))
    AX[:8, 0] = [40.0, -40.0, np.inf, -np.inf, 0.0, -0.0, 745.2, -745.2]
    AX[:4, 4] = [-np.inf, np.inf, -40.0, 40.0]
    got = h(X.weights_block(t(AX)))
    for c in range(k):
        assert same_bytes(got[:, c], h(X.weights(t(AX[:, c]))))
    AXm = h(X.matvec_block(t(rng.standard_normal((prob.d, k)))))
    got = h(X.weights_block(t(AXm)))
    for c in range(k):
        assert same_bytes(got[:, c], h(X.weights(t(AXm[:, c]))))


# --------------------------------------------------------------- 7. fp32 handle
@gpu
def test_fp32_handle(prob):
    """err_block <= 4 err_single + 1e-7 per column: the yardstick is the existing fp32
    krcn_lanczos, measured here against the same fp64 oracle (the same fp32 sums in
    another fixed order give errors of the same order; a wrong expression shows at 1e-1).
    Measured (alphas, betas) per column are printed."""
    f32 = torch.float32
    m, k = 3, 4
    rng = np.random.default_rng(21)
    w = prob.w.astype(np.float32).astype(np.float64)
    G = np.stack([prob.g, prob.s, rng.standard_normal(prob.d), rng.standard_normal(prob.d)], axis=1)
    G = G.astype(np.float32).astype(np.float64)
    X32 = krcn.DeviceCSR(prob.A, dtype=f32)
    V, al, be, infos = X32.lanczos_block(t(w, f32), t(G, f32), m)
    assert V.dtype == f32 and tuple(V.shape) == (m, prob.d, k)
    for c in range(k):
        ref = oracle_column(prob.A, w, G[:, c], m, 0.0)
        _, sal, sbe, si = X32.lanczos(t(w, f32), t(G[:, c], f32), m)
        assert infos[c].m_eff == si.m_eff == m and not infos[c].breakdown
        for name, got, single, exp in (("alphas", al[c], sal, ref["al"]), ("betas", be[c], sbe, ref["be"])):
            err_block, err_single = rel_err(got, exp), rel_err(single, exp)
            print(f"fp32 column {c} {name}: err_block {err_block:.3e} err_single {err_single:.3e}")
            assert err_block <= 4 * err_single + 1e-7


# ---------------------------------------------------------------- 8. workspace
@gpu
def test_workspace_and_no_plan_build(prob):
    n, d = prob.n, prob.d
    W, G, l2 = prob.batch()
    fresh = krcn.DeviceCSR(prob.A).owned_bytes()
    Xw = krcn.DeviceCSR(prob.A)

    def expected(k, m):   # the block HVP's (n, k) intermediate, two (d, k) blocks, partials, results
        return n * k * 8 + 2 * d * k * 8 + PARTIALS_BYTES + k * (2 * m + 3) * 8

    Xw.lanczos_block(t(W[:, :4]), t(G[:, :4]), 5, l2=l2[:4])
    first = Xw.owned_bytes()
    assert first - fresh == expected(4, 5)     # nothing else: no pass plans were built
    Xw.lanczos_block(t(W[:, :4]), t(G[:, :4]), 5, l2=l2[:4])
    assert Xw.owned_bytes() == first
    Xw.lanczos_block(t(W), t(G), 5, l2=l2)
    assert Xw.owned_bytes() > first
    assert Xw.owned_bytes() - fresh == expected(5, 5)
    Xw.lanczos_block(t(W[:, :2]), t(G[:, :2]), 3, l2=l2[:2])
    assert Xw.owned_bytes() - fresh == expected(5, 5)
    # the single-vector paths of the handle are untouched
    wd, gd, sd = t(prob.w), t(prob.g), t(prob.s)
    y0 = h(Xw.hvp(wd, sd, l2=0.01))
    V0, al0, be0, _ = Xw.lanczos(wd, gd, 6)
    V0 = h(V0)
    Xw.lanczos_block(t(W), t(G), 6, l2=l2)
    assert same_bytes(h(Xw.hvp(wd, sd, l2=0.01)), y0)
    V1, al1, be1, _ = Xw.lanczos(wd, gd, 6)
    assert same_bytes(h(V1), V0) and same_bytes(al1, al0) and same_bytes(be1, be0)
    Xw.close()
    assert not Xw.handle.value


@gpu
def test_refusals(prob, X):
    W, G, _ = prob.batch()
    Xs = krcn.DeviceCSR(prob.A, n_global=2 * prob.n, shard_mode=_lib.KRCN_SHARD_ROWS)
    for fn in (lambda: Xs.lanczos_block(t(W), t(G), 3), lambda: Xs.weights_block(t(W)),
               lambda: Xs.basis_combine_block(t(np.zeros((2, prob.d, 5))), np.zeros((2, 5)), t(G))):
        with pytest.raises(_lib.KrcnError) as e:
            fn()
        assert e.value.status == _lib.KRCN_ERR_UNSUPPORTED
    with pytest.raises(_lib.KrcnError) as e:
        X.lanczos_block(t(W[:, :2]), t(G), 3)
    assert e.value.status == _lib.KRCN_ERR_INVALID and "w_cols" in str(e.value)
    with pytest.raises(_lib.KrcnError) as e:
        X.lanczos_block(t(W), t(G), 2045)
    assert e.value.status == _lib.KRCN_ERR_INVALID and "m = 2045" in str(e.value)


# ------------------------------------------------------------ 9. optimizer layer
@gpu
def test_optimizer_layer(f1, prob):
    A, d = prob.A, prob.d
    loss = LogisticRegression(A, f1["b"], l2=0.01)
    Xd = loss.device_matrix
    rng = np.random.default_rng(13)
    G = np.stack([prob.g, prob.s, rng.standard_normal(d)], axis=1)
    xs = np.stack([f1["x0"], f1["x1"], 0.3 * rng.standard_normal(d)], axis=1)
    m = 6
    for label, iterates in (("shared", f1["x0"]), ("per-column", xs)):
        V, al, be, infos = loss.lanczos_block(iterates, G, m)
        assert isinstance(V, np.ndarray) and V.shape == (m, d, 3)
        for c in range(3):
            x = iterates if iterates.ndim == 1 else iterates[:, c]
            w = Xd.weights(Xd.matvec(t(x)))
            _, sal, sbe, si = Xd.lanczos(w, t(G[:, c]), m, l2=0.01)
            assert infos[c].m_eff == si.m_eff and infos[c].hvps == si.hvps
            assert rel_err(al[c], sal) < 1e-11 and rel_err(be[c], sbe) < 1e-11, (label, c)
    Vt, _, _, _ = loss.lanczos_block(t(xs), t(G), m, l2=[0.0, 0.01, 0.02])
    assert isinstance(Vt, torch.Tensor) and Vt.is_cuda and tuple(Vt.shape) == (m, d, 3)
