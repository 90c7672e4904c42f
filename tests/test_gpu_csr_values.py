"""fp32 value storage of the window and jagged plans on fp64 handles
(KRCN_VALUES_F32 / KRCN_VALUES_F32_EXACT, include/krcn.h): only the element
type of a plan's value arrays changes, so a narrowed pass is bitwise the
full-width pass of the same plan over A32 = double(float(A)).

The reference throughout is the existing full-width path and scipy, never the
narrowed code itself.  "FW32" is a values="full" handle with the same format,
lane and slicing policy built over a32(A).  No value of any test matrix is
fp32-exact (asserted when a family is built), so a pass that did not narrow
cannot equal FW32.

Families and the paths they reach:
  jag_short    long_row_matrix() with rows and columns capped at 32, JAG:
               lane-per-row units and the overflow levels; bitwise scipy
  jag_long     long_row_matrix(), JAG: long-row tasks (jlval); 1e-13
  jag_long255  the same capped at 255 elements a row
  jag_acc      45,001 x 61,237, JAG: k_jag_acc in both passes, a tail slice;
               bitwise scipy
  jag_groups   2,500 x 100,000, JAG: slice groups and their combine; 1e-13
  k2, k3, k6   n = 2,000, d = 300,000 / 560,000 / 850,000, two nonzeros a
               column, (WINDOW, JAG): pass 2 has 4,688 / 8,750 / 13,282 row
               groups over 256 blocks, at most 19 / 35 / 52 a block, which
               build_jag turns into k_jag_pass K = 2 / 3 / 6 (plan_info does
               not show K; confirmed by replaying build_jag's balanced cuts
               on the host for these three shapes).  Pass 1 is window slices.
  win_pad      golden f1 padded to 140,000 columns, WINDOW: window slices +
               window accumulate, the early-alpha Lanczos step
  win_jag_pad  the same, (WINDOW, JAG): news20's plan pair
  one_piece    golden f1 (d = 513), WINDOW: SrcLzSmall, EpiLz1X, k_xt_combine

Lanczos against the oracle over a32(A) at the 1e-11 the full-width tests use
for m <= 10: the oracle's own envelope on a32(A) (a 1e-16 relative HVP
perturbation, tests/golden/probe_envelope.py's) is 4.5e-16 / 5.5e-17 (alphas /
betas) on a32(f1) at m = 10, 1.8e-14 / 1.1e-15 with l2 = 0.01, and 2.1e-15 /
2.0e-15 on a32(long_row_matrix()) at m = 12, so no m is dropped.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
import krcn_oracle as O
from conftest import golden_csr, load_golden, rel_err
from krcn import _lib, synth
from optimizer.cubic import Cubic_Krylov_LS
from optimizer.loss import LogisticRegression
from test_gpu_jag import capped_rows
from test_gpu_lanczos import D_PAD, pad_cols
from test_gpu_tiling import long_row_matrix

pytestmark = pytest.mark.gpu

DEV = "cuda"
WAVE, SORTED, WINDOW, JAG, DENSE = (krcn.KRCN_FORMAT_WAVE, krcn.KRCN_FORMAT_SORTED, krcn.KRCN_FORMAT_WINDOW,
                                    krcn.KRCN_FORMAT_JAG, _lib.KRCN_FORMAT_DENSE)
B4, B8 = {"pass1": 4, "pass2": 4}, {"pass1": 8, "pass2": 8}


def t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def h(x):
    torch.cuda.synchronize()
    return x.cpu().numpy()


def a32(A):
    """A with every value rounded to fp32 and widened back."""
    return sp.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices.copy(), A.indptr.copy()),
                         shape=A.shape)


def two_per_column(n, d, seed):
    rng = np.random.default_rng(seed)
    r0 = rng.integers(0, n, size=d)
    r1 = (r0 + 1 + rng.integers(0, n - 1, size=d)) % n   # a second, different row
    rows = np.concatenate([r0, r1])
    cols = np.concatenate([np.arange(d), np.arange(d)])
    A = sp.csr_matrix((rng.uniform(-1, 1, size=2 * d), (rows, cols)), shape=(n, d))
    A.sort_indices()
    return A


def f1_matrix():
    return golden_csr(load_golden("f1_hvp.npz"))


def short_matrix():
    A, _ = long_row_matrix()
    A = capped_rows(capped_rows(A, 32).T.tocsr(), 32).T.tocsr()
    A.sort_indices()
    return A


# name -> (matrix, plan policy, "scipy": bitwise scipy on a32(A) / "tol": 1e-13 against the oracle / None)
FAMILIES = {
    "jag_short": (short_matrix, dict(fmt=JAG), "scipy"),
    "jag_long": (lambda: long_row_matrix()[0], dict(fmt=JAG), "tol"),
    "jag_long255": (lambda: capped_rows(long_row_matrix()[0], 255), dict(fmt=JAG), "tol"),
    "jag_acc": (lambda: synth.make_problem(None, n=45_001, d=61_237, nnz=270_000)[0], dict(fmt=JAG), "scipy"),
    "jag_groups": (lambda: synth.make_problem(None, n=2500, d=100_000, nnz=30_000)[0], dict(fmt=JAG), "tol"),
    "k2": (lambda: two_per_column(2000, 300_000, 2), dict(pass_formats=(WINDOW, JAG)), None),
    "k3": (lambda: two_per_column(2000, 560_000, 3), dict(pass_formats=(WINDOW, JAG)), None),
    "k6": (lambda: two_per_column(2000, 850_000, 6), dict(pass_formats=(WINDOW, JAG)), None),
    "win_pad": (lambda: pad_cols(f1_matrix(), D_PAD), dict(fmt=WINDOW), None),
    "win_jag_pad": (lambda: pad_cols(f1_matrix(), D_PAD), dict(pass_formats=(WINDOW, JAG)), None),
    "one_piece": (f1_matrix, dict(fmt=WINDOW), None),
}
EXPECT_FORMAT = {
    "jag_short": ("jagged", "jagged"), "jag_long": ("jagged", "jagged"), "jag_long255": ("jagged", "jagged"),
    "jag_acc": ("jagged", "jagged"), "jag_groups": ("jagged", "jagged"),
    "k2": ("window-slices", "jagged"), "k3": ("window-slices", "jagged"), "k6": ("window-slices", "jagged"),
    "win_pad": ("window-slices", "window-accum"), "win_jag_pad": ("window-slices", "jagged"),
    "one_piece": ("window-accum", "window-accum"),
}


class Family:
    """The three handles of one family over the same policy, their plans built
    (and owned bytes read) before any compute call, and shared inputs."""

    def __init__(self, name):
        make, self.policy, self.order = FAMILIES[name]
        self.name = name
        self.A = sp.csr_matrix(make())
        self.A32 = a32(self.A)
        assert not np.array_equal(self.A32.data, self.A.data)
        self.full = krcn.DeviceCSR(self.A, values="full", **self.policy)
        self.nar = krcn.DeviceCSR(self.A, values="f32", **self.policy)
        self.fw32 = krcn.DeviceCSR(self.A32, values="full", **self.policy)
        self.info = {k: (X.plan_format(), X.plan_info(), X.plan_value_bytes(), X.owned_bytes())
                     for k, X in (("full", self.full), ("nar", self.nar), ("fw32", self.fw32))}
        n, d = self.A.shape
        rng = np.random.default_rng(len(name))
        self.x = rng.uniform(-0.3, 0.3, size=d)
        self.v = rng.standard_normal(d)
        self.u = rng.standard_normal(n)
        self.b01 = (rng.uniform(size=n) < 0.5).astype(np.float64)
        self.w = O.hessian_weights(self.A32, self.x)

    def outputs(self, X):
        """matvec, rmatvec, hvp at l2 = 0 and 0.01, gradient (l2 = 0 and 0.01), loss_values, cg_solve."""
        x, v, u, w, b = t(self.x), t(self.v), t(self.u), t(self.w), t(self.b01)
        Ax = X.matvec(x)
        sol, ci = X.cg_solve(w, v, shift=0.05, rtol=1e-12, maxiter=6)
        out = [h(Ax), h(X.rmatvec(u)), h(X.hvp(w, v)), h(X.hvp(w, v, l2=0.01)), h(X.gradient(Ax, b)),
               h(X.gradient(Ax, b, x, l2=0.01)), np.array(X.loss_values([x, v * 0.1], b)), h(sol),
               np.array([ci.converged, ci.info, ci.iterations, ci.residual_norm])]
        return out


_FAMILIES = {}


def family(name):
    """Built once a module run and shared read-only (the matrices are small)."""
    if name not in _FAMILIES:
        _FAMILIES[name] = Family(name)
    return _FAMILIES[name]


@pytest.fixture(scope="module", params=sorted(FAMILIES))
def fam(request):
    return family(request.param)


@pytest.fixture(scope="module")
def win_jag():
    return family("win_jag_pad")


def assert_same(got, ref, what=""):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what} output {k}")


# ------------------------------------------------------------ 1. reporting
def test_reporting(fam):
    """The narrowed handle reports 4 / 4, the format and plan summary of the
    full-width handle, and owns at least 8 nnz fewer bytes: each pass stores at
    least nnz values and each shrinks by 4 bytes.  (Fails without the feature.)"""
    ffmt, finfo, fvb, fown = fam.info["full"]
    nfmt, ninfo, nvb, nown = fam.info["nar"]
    assert (ffmt["pass1"], ffmt["pass2"]) == EXPECT_FORMAT[fam.name]
    assert fvb == B8 and fam.info["fw32"][2] == B8
    assert nvb == B4
    assert nfmt == ffmt and ninfo == finfo
    assert fam.info["fw32"][:2] == (ffmt, finfo)
    assert fown - nown >= 8 * fam.A.nnz
    assert fam.info["fw32"][3] == fown


# ------------------------------------------- 2. / 3. bitwise against FW32
def test_bitwise_against_full_width_over_a32(fam):
    got = fam.outputs(fam.nar)
    assert_same(got, fam.outputs(fam.fw32), fam.name)
    A32, n = fam.A32, fam.A.shape[0]
    refs = [A32 @ fam.x, (A32.T @ fam.u) / n, O.hvp_from_weights(A32, fam.w, fam.v),
            O.hvp_from_weights(A32, fam.w, fam.v, l2=0.01)]
    if fam.order == "scipy":
        assert_same(got[:4], refs, fam.name + " scipy")
    elif fam.order == "tol":
        for y, r in zip(got[:4], refs):
            assert rel_err(y, r) < 1e-13


def test_it_really_rounds(fam):
    y = h(fam.nar.matvec(t(fam.x)))
    y_full = h(fam.full.matvec(t(fam.x)))
    assert not np.array_equal(y, y_full)
    assert rel_err(y, y_full) < 1e-6   # (fp32 rounding of the values: 6e-8 a product)


# ------------------------------------------------ 4. Lanczos against FW32
INFO_FIELDS = ("m_eff", "breakdown", "j_break", "hvps", "beta_last", "gnorm")


def lanczos_pair(Xa, Xb, w, g, m, l2=0.0):
    Va, ala, bea, ia = Xa.lanczos(w, g, m, l2=l2)
    Va = h(Va)[:ia.m_eff].copy()
    Vb, alb, beb, ib = Xb.lanczos(w, g, m, l2=l2)
    Vb = h(Vb)[:ib.m_eff]
    for f in INFO_FIELDS:
        assert getattr(ia, f) == getattr(ib, f), f
    np.testing.assert_array_equal(ala, alb)
    np.testing.assert_array_equal(bea, beb)
    np.testing.assert_array_equal(Va, Vb)
    return ala, bea, ia


LZ_PLANS = {"win_pad": (dict(fmt=WINDOW), D_PAD), "win_jag_pad": (dict(pass_formats=(WINDOW, JAG)), D_PAD),
            "one_piece": (dict(fmt=WINDOW), None)}


def lz_problem(A0, b, x0, plan):
    """(narrowed handle, FW32 handle, w, g, w and g on the host) of A0 under LZ_PLANS[plan]; w and g
    are the oracle's over a32(A0) (columns padded with empty ones as test_gpu_lanczos.py does)."""
    policy, dpad = LZ_PLANS[plan]
    B0 = a32(A0)
    assert not np.array_equal(B0.data, A0.data)
    wh = O.hessian_weights(B0, x0)
    gh = O.gradient(B0, O.labels01(b), x0)
    A, B, gp = A0, B0, gh
    if dpad:
        A, B = pad_cols(A0, dpad), pad_cols(B0, dpad)
        gp = np.concatenate([gh, np.zeros(dpad - A0.shape[1])])
    nar = krcn.DeviceCSR(A, values="f32", **policy)
    fw32 = krcn.DeviceCSR(B, values="full", **policy)
    assert nar.plan_value_bytes() == B4 and fw32.plan_value_bytes() == B8
    assert nar.plan_format() == fw32.plan_format()
    return nar, fw32, t(wh), t(gp), B0, wh, gh


@pytest.mark.parametrize("plan", sorted(LZ_PLANS))
def test_lanczos_bitwise_and_against_oracle(plan):
    f1 = load_golden("f1_hvp.npz")
    nar, fw32, w, g, B0, wh, gh = lz_problem(golden_csr(f1), f1["b"], f1["x0"], plan)
    for l2 in (0.0, 0.01):
        for m in (1, 10):
            al, be, info = lanczos_pair(nar, fw32, w, g, m, l2)
            assert info.m_eff == m and not info.breakdown
            _, al_r, be_r, _ = O.lanczos(lambda q: O.hvp_from_weights(B0, wh, q, l2=l2), gh, m)
            assert rel_err(al, al_r) < 1e-11 and rel_err(be, be_r) < 1e-11


@pytest.mark.parametrize("plan", sorted(LZ_PLANS))
@pytest.mark.parametrize("r,ms", [(1, (2, 3, 5)), (3, (4, 5, 10))])
def test_lanczos_breakdown_cases_bitwise(plan, r, ms):
    """Golden f2's rank-r operators (the recurrence ends early or runs on
    rounding residue): whatever a32 makes of them, the narrowed handle and
    FW32 agree in every output and every field of the info."""
    f2 = load_golden("f2_lanczos.npz")
    A0 = golden_csr(f2, f"r{r}_")
    nar, fw32, w, g, *_ = lz_problem(A0, f2[f"r{r}_b"], np.full(A0.shape[1], 0.5), plan)
    for m in ms:
        lanczos_pair(nar, fw32, w, g, m)


def test_lanczos_long_rows_bitwise_and_against_oracle():
    fam = family("jag_long")
    g = np.random.default_rng(12).standard_normal(fam.A.shape[1])
    al, be, _ = lanczos_pair(fam.nar, fam.fw32, t(fam.w), t(g), 12)
    _, al_r, be_r, _ = O.lanczos(lambda q: O.hvp_from_weights(fam.A32, fam.w, q), g, 12)
    assert rel_err(al, al_r) < 1e-11 and rel_err(be, be_r) < 1e-11


# ------------------------------------------------------ 5. both or neither
def small_outputs(X, u, v, w):
    return [h(X.matvec(t(v))), h(X.rmatvec(t(u))), h(X.hvp(t(w), t(v))), h(X.hvp(t(w), t(v), l2=0.01))]


@pytest.fixture(scope="module")
def f1_inputs():
    A = f1_matrix()
    rng = np.random.default_rng(5)
    return A, rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[1]), rng.uniform(0.01, 0.25, A.shape[0])


@pytest.mark.parametrize("formats", [(SORTED, JAG), (WAVE, WINDOW)])
def test_a_csr_pass_beside_a_full_width_one_stays_full(f1_inputs, formats):
    A, u, v, w = f1_inputs
    nar = krcn.DeviceCSR(A, pass_formats=formats, values="f32")
    full = krcn.DeviceCSR(A, pass_formats=formats, values="full")
    assert nar.plan_value_bytes() == B8
    assert nar.plan_format() == full.plan_format() and nar.plan_info() == full.plan_info()
    assert nar.owned_bytes() == full.owned_bytes()
    assert_same(small_outputs(nar, u, v, w), small_outputs(full, u, v, w))


@pytest.mark.parametrize("formats", [(DENSE, JAG), (WINDOW, DENSE)])
def test_a_csr_pass_beside_a_dense_one_narrows(f1_inputs, formats):
    """A narrowed dense image takes the geometry of 4-byte entries (lanes from
    ceil(cols / 4) vectors, include/krcn.h), so under the automatic lane policy
    its sums are not in FW32's order: there the CSR pass's own output is
    bitwise FW32's and the dense pass's within 1e-13 of the oracle over a32(A).
    Under the sequential lane policy both widths of a dense pass are scipy's
    order, and every output is bitwise FW32's."""
    A, u, v, w = f1_inputs
    B = a32(A)
    for lanes in ((1, 1), (0, 0)):
        nar = krcn.DeviceCSR(A, pass_formats=formats, values="f32", lanes=lanes)
        fw32 = krcn.DeviceCSR(B, pass_formats=formats, values="full", lanes=lanes)
        assert nar.plan_value_bytes() == B4 and fw32.plan_value_bytes() == B8
        assert nar.plan_format() == fw32.plan_format()
        got, ref = small_outputs(nar, u, v, w), small_outputs(fw32, u, v, w)
        if lanes == (1, 1):
            assert_same(got, ref)
            continue
        csr = 1 if formats[1] != DENSE else 0   # rmatvec runs pass 2, matvec pass 1
        np.testing.assert_array_equal(got[csr], ref[csr])
        oracle = [B @ v, (B.T @ u) / A.shape[0], O.hvp_from_weights(B, w, v), O.hvp_from_weights(B, w, v, l2=0.01)]
        for y, r in zip(got, oracle):
            assert rel_err(y, r) < 1e-13


# ----------------------------------------------------------- 6. f32-exact
def test_f32_exact(win_jag):
    A = win_jag.A
    E = A.copy()
    E.data = np.where(np.round(A.data * 8) == 0, 1.0, np.round(A.data * 8)) / 8   # multiples of 1/8, none zero
    assert np.array_equal(a32(E).data, E.data)
    u, v, w = win_jag.u, win_jag.v, win_jag.w
    ex = krcn.DeviceCSR(E, values="f32-exact", **win_jag.policy)
    full = krcn.DeviceCSR(E, values="full", **win_jag.policy)
    assert ex.plan_value_bytes() == B4 and ex.plan_format() == full.plan_format()
    assert full.owned_bytes() - ex.owned_bytes() >= 8 * E.nnz
    assert_same(small_outputs(ex, u, v, w), small_outputs(full, u, v, w))
    inexact = krcn.DeviceCSR(A, values="f32-exact", **win_jag.policy)
    assert inexact.plan_value_bytes() == B8 and inexact.owned_bytes() == win_jag.info["full"][3]
    assert_same(small_outputs(inexact, u, v, w), small_outputs(win_jag.full, u, v, w))
    N = E.copy()
    N.data[7] = np.nan
    assert krcn.DeviceCSR(N, values="f32-exact", **win_jag.policy).plan_value_bytes() == B8


# ---------------------------------------------------------- 7. fp32 handle
def test_fp32_handle_policy_is_a_no_op(win_jag):
    u, v, w = (t(a, torch.float32) for a in (win_jag.u, win_jag.v, win_jag.w))
    got = []
    for values in ("full", "f32", "f32-exact"):
        X = krcn.DeviceCSR(win_jag.A, dtype=torch.float32, values=values, **win_jag.policy)
        assert X.plan_value_bytes() == B4
        got.append((X.plan_format(), X.plan_info(), X.owned_bytes(), h(X.matvec(v)), h(X.rmatvec(u)), h(X.hvp(w, v))))
    for g in got[1:]:
        assert g[:3] == got[0][:3]
        assert_same(g[3:], got[0][3:])


# ----------------------------------------------------------- 8. re-planning
def test_replanning(win_jag):
    A, u, v, w = win_jag.A, win_jag.u, win_jag.v, win_jag.w
    X = krcn.DeviceCSR(A, values="f32", **win_jag.policy)
    X.plan_info()
    own = X.owned_bytes()
    ref = small_outputs(win_jag.fw32, u, v, w)
    assert_same(small_outputs(X, u, v, w), ref)
    own_used = X.owned_bytes()
    X.set_value_storage("full")
    assert X.plan_value_bytes() == B8 and X.owned_bytes() - own_used >= 8 * A.nnz
    X.set_value_storage("f32")
    assert X.plan_value_bytes() == B4 and X.owned_bytes() == own_used >= own
    assert_same(small_outputs(X, u, v, w), ref)
    X.set_placement_trials(2)
    assert X.plan_value_bytes() == B4 and X.placement_info()["probed"] == 2
    assert_same(small_outputs(X, u, v, w), ref)


def test_graph_replay_bitwise(win_jag):
    X = win_jag.nar
    g = t(np.random.default_rng(3).standard_normal(X.d))
    w = t(win_jag.w)
    V = torch.empty((10, X.d), dtype=X.dtype, device=DEV)
    X.set_graph(False)
    for _ in range(2):
        _, al0, be0, _ = X.lanczos(w, g, 10, V=V)
    V0 = V.clone()
    X.set_graph(True)
    try:
        for k in range(3):   # eager (new key) -> record + launch -> replay
            _, al, be, _ = X.lanczos(w, g, 10, V=V)
            np.testing.assert_array_equal(al, al0, err_msg=f"call {k}")
            np.testing.assert_array_equal(be, be0, err_msg=f"call {k}")
            assert torch.equal(V, V0), k
    finally:
        X.set_graph(False)


# ------------------------------------------------------ 9. coordinate calls
@pytest.mark.parametrize("name", ["one_piece", "jag_short", "win_jag_pad"])
def test_coordinate_calls_read_full_width_values(name):
    """The documented split: the coordinate calls read the handle's transposed
    CSR, which stays full width: bitwise a full-width handle's over A."""
    fam = family(name)
    nar, full = fam.nar, fam.full
    x, b = t(fam.x), t(fam.b01)
    Ax = full.matvec(x)
    cols = np.flatnonzero(np.diff(fam.A.tocsc().indptr))[:48]
    delta = np.linspace(-0.5, 0.5, len(cols))
    np.testing.assert_array_equal(nar.coord_gradient(cols, Ax, b), full.coord_gradient(cols, Ax, b))
    np.testing.assert_array_equal(nar.coord_hessian(cols, Ax, l2=0.01), full.coord_hessian(cols, Ax, l2=0.01))
    np.testing.assert_array_equal(h(nar.coord_update(cols, delta, Ax)), h(full.coord_update(cols, delta, Ax)))
    _, _, vals = nar.transpose_arrays()
    np.testing.assert_array_equal(np.sort(h(vals)), np.sort(fam.A.data))


# ---------------------------------------------------- 10. LogisticRegression
def test_loss_accepts_narrowed_values_with_a_named_format():
    f1 = load_golden("f1_hvp.npz")
    A = pad_cols(golden_csr(f1), D_PAD)
    # (the jagged format does not take the padded matrix's 16 column slices: f1 as it is)
    for M, fmt in ((A, "auto"), (A, WINDOW), (golden_csr(f1), JAG)):
        loss = LogisticRegression(M, f1["b"], l1=0, l2=0, format=fmt, values="f32")
        vb = loss.device_matrix.plan_value_bytes()
        assert vb == B4 if fmt != "auto" else vb in (B4, B8)
    with pytest.raises(ValueError):
        LogisticRegression(A, f1["b"], l1=0, l2=0, values="f32")
    for fmt in (WAVE, SORTED):
        with pytest.raises(ValueError):
            LogisticRegression(A, f1["b"], l1=0, l2=0, format=fmt, values="f32")
    assert LogisticRegression(A, f1["b"], l1=0, l2=0, format="auto").device_matrix.plan_value_bytes() == B8


def test_krylov_crn_run_equals_full_width_over_a32():
    f1 = load_golden("f1_hvp.npz")
    A = pad_cols(golden_csr(f1), D_PAD)
    runs = []
    for M, values in ((A, "f32"), (a32(A), "full")):
        loss = LogisticRegression(M, f1["b"], l1=0, l2=0, store_mat_vec_prod=True, format=WINDOW, values=values)
        assert loss.device_matrix.plan_value_bytes() == (B4 if values == "f32" else B8)
        assert loss.device_matrix.plan_format()["pass1"] == "window-slices"
        opt = Cubic_Krylov_LS(loss=loss, reg_coef=1e-3, label="krylov", subspace_dim=10, tolerance=1e-9, tqdm=False)
        tr = opt.run(x0=np.concatenate([f1["x0"], np.zeros(D_PAD - len(f1["x0"]))]), it_max=5)
        opt.compute_loss_of_iterates()
        runs.append((np.asarray(tr.xs), np.asarray(tr.loss_vals), list(tr.solver_its), opt.reg_coef))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert runs[0][2:] == runs[1][2:]
