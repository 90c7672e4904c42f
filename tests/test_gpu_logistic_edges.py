"""The logistic scalar layer of the kernels (expit, logsig; k_weights,
k_residual, k_loss_terms and its guarded copy; the coordinate kernels) at
saturated margins, element by element, against the 300-bit reference of
tests/logistic_ref.py.

Accuracy: on the margin grid a device function may exceed the exact value by
what the reference's numpy formula does on the same grid (computed here) plus
2 ulp: one per library call (exp, log1p) in which the device library may
differ from glibc.  The +2 is not a measurement; DESIGN.md §4 carries what an
MI355X gives.  Weights are scaled by expit, the b = 1 residual by 1, loss
terms by max(|a|, |t|) (tests/test_logistic_reference.py says why).

The margins go in directly: weights / gradient / loss_mean take Ax.  With
X = I (8192 x 8192) and l2 = 0, gradient * 8192 is the residual; loss terms
come one by one from a 1 x 1 handle's loss_values.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.special
import torch

import krcn
import krcn_oracle as O
import logistic_ref as R
from conftest import rel_err
from krcn import synth
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ID = 8192
DTYPES = {"fp64": (np.float64, torch.float64), "fp32": (np.float32, torch.float32)}


def t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def h(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module", params=list(DTYPES), ids=list(DTYPES))
def ctx(request):
    """Per dtype: the grid with its exact values and numpy excesses, the identity
    handle, the 1 x 1 handle, and the device's weights / residuals / loss terms."""
    npdt, tdt = DTYPES[request.param]
    x, table = R.reference_excesses(npdt)
    ident = krcn.DeviceCSR(sp.identity(N_ID, format="csr"), dtype=tdt)
    one = krcn.DeviceCSR(sp.csr_matrix(np.ones((1, 1))), dtype=tdt)
    pad = np.zeros(N_ID, dtype=npdt)
    pad[:len(x)] = x
    Ax = t(pad, tdt)
    G = len(x)
    dev = {"weights": h(ident.weights(Ax))[:G]}
    for b in (0, 1):
        g = ident.gradient(Ax, torch.full((N_ID,), float(b), dtype=tdt, device=DEV))
        dev[f"residual_b{b}"] = h(g * N_ID)[:G]
    dev["loss_b0"] = loss_terms(one, x, 0.0, tdt)
    dev["loss_b1"] = loss_terms(one, x, 1.0, tdt)
    yield dict(name=request.param, npdt=npdt, tdt=tdt, x=x, table=table, ident=ident, one=one, dev=dev)
    ident.close()
    one.close()


def loss_terms(one, x, b, tdt):
    """(1 - b) x_i - logsig(x_i) per element: loss_values of the 1 x 1 handle X = [1]
    (Ax = x, a mean over one row), every value a T widened to double."""
    xs = t(x, tdt)
    bd = torch.full((1,), b, dtype=tdt, device=DEV)
    vals = np.array(one.loss_values([xs[i:i + 1] for i in range(len(x))], bd))
    out = vals.astype(x.dtype)
    assert np.array_equal(out.astype(np.float64), vals, equal_nan=True)
    return out


# ----------------------------------------------------------------- accuracy
CASES = [("weights", "weights"), ("residual_b0", "expit"), ("residual_b1", "residual_b1"),
         ("loss_b0", "loss_b0"), ("loss_b1", "loss_b1")]


@pytest.mark.parametrize("fn,key", CASES, ids=[c[0] for c in CASES])
def test_accuracy_on_the_margin_grid(ctx, fn, key):
    np_excess, exact, scale = ctx["table"][key]
    got = ctx["dev"][fn]
    assert got.dtype == np.dtype(ctx["npdt"]) and not np.isnan(got).any()
    e = R.excess(got, exact, ctx["npdt"], scale)
    print(f"{ctx['name']} {fn}: device excess {e:.2f} ulp, numpy formula {np_excess:.2f} ulp, bound {np_excess + 2:.2f}")
    assert np_excess <= 3.0
    assert e <= np_excess + 2.0


def test_device_logsig_in_ulps_of_itself(ctx):
    """The b = 1 term is (1 - 1) a - logsig(a) = -logsig(a) with no rounding of its
    own, so the device's logsig is read off it and held to ulps of |logsig(a)|
    (not of |a|): the outer branch -exp(-a) and the tail of log1p(exp(-a)), which
    ulps of a >= 37 would hide, against the numpy logsig's excess + 2."""
    np_excess, exact, _ = ctx["table"]["logsig"]
    assert np.array_equal(R.np_loss_term(ctx["x"], 1), -R.np_logsig(ctx["x"]))
    e = R.excess(-ctx["dev"]["loss_b1"], exact, ctx["npdt"])
    print(f"{ctx['name']} logsig: device excess {e:.2f} ulp, numpy formula {np_excess:.2f} ulp, bound {np_excess + 2:.2f}")
    assert np_excess <= 3.0
    assert e <= np_excess + 2.0


def test_loss_mean_of_64_terms(ctx):
    """A 64-row handle's loss_mean over margins from every branch: the sum of the
    per-element terms in double, over 64 (one wave; b alternates)."""
    npdt, tdt = ctx["npdt"], ctx["tdt"]
    x = ctx["x"]
    pick = x[np.linspace(0, len(x) - 1, 64).astype(int)]
    b = (np.arange(64) % 2).astype(npdt)
    X = krcn.DeviceCSR(sp.identity(64, format="csr"), dtype=tdt)
    got = X.loss_mean(t(pick, tdt), t(b, tdt))
    terms = np.where(b == 0, R.np_loss_term(pick, 0), R.np_loss_term(pick, 1)).astype(np.float64)
    exact = [a if bi == 0 else c for bi, a, c in zip(b, R.exact_loss_term(pick, 0), R.exact_loss_term(pick, 1))]
    with R.mp.workprec(R.PREC):
        want = float(sum(exact) / 64)
    # every term within (numpy excess + 2) ulp of max(|a|, |t|) <= 2 * 746; 64 of them, then one mean
    worst = max(ctx["table"]["loss_b0"][0], ctx["table"]["loss_b1"][0]) + 2
    bound = worst * sum(float(R.ulp(s, npdt)) for s in R.loss_scale(pick, exact)) / 64 + 64 * np.finfo(np.float64).eps * abs(want) \
        + float(np.finfo(npdt).tiny)
    print(f"{ctx['name']}: loss_mean of 64 terms {got!r}, exact {want!r}, |diff| {abs(got - want):.3e}, bound {bound:.3e}; "
          f"numpy {terms.sum() / 64!r}")
    assert abs(got - want) <= bound
    X.close()


# ----------------------------------------------------------- branch identity
def test_branch_identities(ctx):
    """Below -33 logsig(a) is a itself: the b = 1 term is exactly -a, the b = 0
    term exactly 0 (both dtypes run the fp64 thresholds).  In [-33, -18) the
    term is -(a - exp(a)) for b = 1: exp(a) <= e^-18 carries a library
    difference of an ulp of itself, 2^-52 e^-18 (fp32: 2^-23 e^-18), far below
    half an ulp of a, so the rounded difference is the correctly rounded one
    wherever the exact value is not within 1e-6 ulp of a tie."""
    x, npdt = ctx["x"], ctx["npdt"]
    l0, l1 = ctx["dev"]["loss_b0"], ctx["dev"]["loss_b1"]
    low = x < -33
    assert low.sum() > 500
    assert np.array_equal(l1[low], -x[low])
    assert np.array_equal(l0[low], np.zeros(low.sum(), dtype=npdt))
    mid = np.flatnonzero((x >= -33) & (x < -18))
    assert len(mid) > 500
    checked = differ = 0
    for i, v in zip(mid, R.exact_mid_branch(x[mid])):
        if R.tie_distance(v, npdt) < 1e-6:
            continue
        want = -R.round_to(v, npdt)
        assert l1[i] == want, (x[i], l1[i], want)
        checked += 1
        differ += want != -x[i]
    assert checked > 500
    # the exp(a) term is visible in fp64 down to about -33 (in fp32 it is below half an ulp of a throughout)
    if npdt == np.float64:
        assert differ > 0.9 * checked


@pytest.mark.parametrize("th", [-33.0, -18.0, 37.0])
def test_single_elements_around_each_threshold(ctx, th):
    """One element below, at and above each threshold, each against the exact
    value of the branch the reference takes for it, and against the oracle."""
    npdt, tdt = ctx["npdt"], ctx["tdt"]
    v = npdt(th)
    pts = np.array([np.nextafter(v, npdt(-np.inf)), v, np.nextafter(v, npdt(np.inf))], dtype=npdt)

    def branch(a):
        a = R.mpf(float(a))
        if a < -33:
            return a
        if a < -18:
            return a - R.mpmath.exp(a)
        if a < 37:
            return -R.mpmath.log1p(R.mpmath.exp(-a))
        return -R.mpmath.exp(-a)

    for b in (0, 1):
        got = loss_terms(ctx["one"], pts, float(b), tdt)
        ref = R.np_loss_term(pts, b)
        with R.mp.workprec(R.PREC):
            ls = [branch(a) for a in pts]
            exact = [(1 - b) * R.mpf(float(a)) - l for a, l in zip(pts, ls)]
            # b = 1: the term is -logsig(a) with no rounding of its own, held to ulps of itself
            scale = [abs(e) if b == 1 else max(abs(R.mpf(float(a))), abs(l), abs(e)) for a, l, e in zip(pts, ls, exact)]
        e_dev = R.excess(got, exact, npdt, scale)
        e_np = R.excess(ref, exact, npdt, scale)
        print(f"{ctx['name']} threshold {th} b={b}: device {got.tolist()}, numpy {ref.tolist()}, "
              f"excess {e_dev:.2f} (numpy {e_np:.2f})")
        assert e_dev <= e_np + 2.0
        if th == -33.0:
            want = -pts[0] if b == 1 else npdt(0)
            assert got[0] == want
            if b == 0 and npdt == np.float64:
                # at and above -33 the branch a - exp(a) is taken: a - fl(a - exp(a)) is exp(a) to an ulp of a, not 0
                assert got[1] != 0 and got[2] != 0


def test_above_37_b0_is_a_plus_exp_minus_a(ctx):
    x, npdt = ctx["x"], ctx["npdt"]
    hi = x >= 37
    assert hi.sum() > 500
    with np.errstate(under="ignore"):
        want = x[hi] + np.exp(-x[hi])
    got = ctx["dev"]["loss_b0"][hi]
    # exp(-a) <= e^-37 is below half an ulp of a >= 37 in both dtypes: the sum rounds to a
    assert np.array_equal(want, x[hi])
    assert np.array_equal(got, want)


# ------------------------------------------------- saturation and non-finite
def test_saturated_weights(ctx):
    x, npdt, tdt = ctx["x"], ctx["npdt"], ctx["tdt"]
    w = ctx["dev"]["weights"]
    ref = R.np_weights(x)
    assert (ref == 0).sum() > 500
    assert (w[ref == 0] == 0).all()
    assert (w >= 0).all() and (w <= 0.25).all()
    assert w[x == 0][0] == 0.25
    one = ctx["one"]
    for v in (np.inf, -np.inf):
        assert h(one.weights(t(np.array([v], dtype=npdt), tdt)))[0] == 0
    r = ctx["dev"]["residual_b0"]
    assert (r >= 0).all() and (r <= 1).all()
    low = r[x <= -746]
    assert len(low) >= 2 and (low < np.finfo(npdt).tiny).all()


def test_nan_is_not_dropped(ctx):
    npdt, tdt, ident = ctx["npdt"], ctx["tdt"], ctx["ident"]
    Ax = np.zeros(N_ID, dtype=npdt)
    Ax[4097] = np.nan
    w = h(ident.weights(t(Ax, tdt)))
    assert np.isnan(w[4097]) and np.isnan(w).sum() == 1
    for b in (0.0, 1.0):
        assert np.isnan(ident.loss_mean(t(Ax, tdt), torch.full((N_ID,), b, dtype=tdt, device=DEV)))
    g = h(ident.gradient(t(Ax, tdt), torch.zeros(N_ID, dtype=tdt, device=DEV)))
    assert np.isnan(g[4097]) and np.isnan(g).sum() == 1


def test_residuals_finite_where_exp_overflows(ctx):
    """exp(-x) is inf in fp32 below -88.7 (fp64: -709.8): expit is 0 there, not NaN."""
    npdt, tdt, ident = ctx["npdt"], ctx["tdt"], ctx["ident"]
    lo, hi = (-104, -88) if npdt == np.float32 else (-746, -708)
    Ax = np.zeros(N_ID, dtype=npdt)
    Ax[:4001] = np.linspace(lo, hi, 4001).astype(npdt)
    for b in (0.0, 1.0):
        g = h(ident.gradient(t(Ax, tdt), torch.full((N_ID,), b, dtype=tdt, device=DEV)) * N_ID)
        assert np.isfinite(g).all()
        assert np.abs(g[:4001] + npdt(b)).max() <= 2 * np.finfo(npdt).tiny


# -------------------------------------- one formula, several copies: bitwise
@pytest.fixture(scope="module")
def saturated():
    """300 x 5003 with x scaled until |Ax| passes 40 on both sides; every logsig branch has rows."""
    A, b = synth.make_problem(None, seed=11, n=300, d=5003, nnz=9000)
    x = np.random.default_rng(5).standard_normal(A.shape[1])
    Ax = A @ x
    x *= 60.0 / min(Ax.max(), -Ax.min())
    Ax = A @ x
    assert (Ax > 40).sum() >= 3 and (Ax < -40).sum() >= 3 and (np.abs(Ax) < 18).sum() >= 30
    assert min(branch_rows(Ax)) >= 3
    return A, b, x


def branch_rows(Ax):
    """Rows in each logsig branch: below -33, [-33, -18), [-18, 37), 37 and above."""
    Ax = np.asarray(Ax, dtype=np.float64)
    return [int((Ax < -33).sum()), int(((Ax >= -33) & (Ax < -18)).sum()), int(((Ax >= -18) & (Ax < 37)).sum()),
            int((Ax >= 37).sum())]


@pytest.mark.parametrize("dt", list(DTYPES))
def test_loss_values_is_loss_mean_on_saturated_iterates(saturated, dt):
    npdt, tdt = DTYPES[dt]
    A, b, x = saturated
    X = krcn.DeviceCSR(A, dtype=tdt)
    bd = t(O.labels01(b).astype(npdt), tdt)
    xs = [t(x.astype(npdt), tdt), t((-0.7 * x).astype(npdt), tdt), t((1.5 * x).astype(npdt), tdt)]
    for v in xs:
        assert min(branch_rows(h(X.matvec(v)))) >= 1
    singles = [X.loss_mean(X.matvec(v), bd) for v in xs]
    assert X.loss_values(xs, bd) == singles
    # and the value is the oracle's (the terms differ from numpy's by ulps of |Ax| at most)
    if npdt == np.float64:
        for v, s in zip(xs, singles):
            want = O.value(A, O.labels01(b), h(v))
            assert abs(s - want) <= 1e-13 * abs(want)
    X.close()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("l2", [0.0, 0.01])
def test_crn_step_value_is_loss_mean_on_a_saturated_iterate(saturated, l2, dt):
    """value_new of the device step (k_loss_terms_guard inside the chain) against
    krcn_loss_mean of the iterate it returns, with the l2 term formed as
    LogisticRegression._value forms it."""
    A, b, x = saturated
    loss = LogisticRegression(A, b, l1=0, l2=l2, store_mat_vec_prod=True, dtype=DTYPES[dt][1])
    X = loss.device_matrix
    xd = loss.to_device(x)
    keep = xd.clone()
    value = loss.value(xd)
    x_new, Ax_new, al, be, info = X.crn_step(xd, loss._b_dev, value, 10, 1e-3, Ax=loss._device_Ax(xd), l2=l2)
    assert torch.equal(xd, keep)
    want = X.loss_mean(X.matvec(x_new), loss._b_dev)
    if l2 != 0:
        want = want + l2 / 2 * X.diff_norm(x_new) ** 2
    print(f"{dt} l2 {l2}: accepted {info.accepted} after {info.trials} backtracking trials, value {value!r} -> {info.value_new!r}")
    assert np.isfinite(info.value_new)
    assert info.value_new == want
    assert torch.equal(Ax_new, X.matvec(x_new))
    rows = branch_rows(h(Ax_new))
    print(f"rows of Ax_new per logsig branch: {rows}")
    assert min(rows) >= 1          # the guarded loss kernel ran every branch
    if info.accepted:
        assert info.value_new <= value - info.model_decrease
    else:
        assert info.trials == 20 and info.value_new > value - info.model_decrease


@pytest.mark.parametrize("dt", list(DTYPES))
def test_coordinate_kernels_on_a_saturated_iterate(saturated, dt):
    npdt, tdt = DTYPES[dt]
    tol = 1e-13 if npdt == np.float64 else 1e-5
    A, b, x = saturated
    n = A.shape[0]
    b01 = O.labels01(b)
    Ax = A @ x
    cols = np.unique(A[np.flatnonzero(np.abs(Ax) > 40)].indices)[:8]     # columns that saturated rows touch
    assert len(cols) == 8
    C = A.tocsc()[:, cols]
    w = O.hessian_weights(A, x)
    assert (w == 0).sum() >= 3
    g_ref = C.T @ (scipy.special.expit(Ax) - b01) / n
    H_ref = (C.T.multiply(w) @ C / n).toarray()
    X = krcn.DeviceCSR(A, dtype=tdt)
    Axd, bd = t(Ax.astype(npdt), tdt), t(b01.astype(npdt), tdt)
    eg = rel_err(X.coord_gradient(cols, Axd, bd), g_ref)
    eh = rel_err(X.coord_hessian(cols, Axd), H_ref)
    print(f"{dt}: saturated coord gradient rel err {eg:.3e}, hessian rel err {eh:.3e}")
    assert eg < tol
    assert eh < tol
    X.close()


def test_hvp_with_half_the_weights_zero(saturated):
    A, b, x = saturated
    n, d = A.shape
    rng = np.random.default_rng(9)
    Ax = np.where(rng.random(n) < 0.5, rng.uniform(37, 700, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-3, 3, n))
    Ax[Ax < -36] -= 710.0          # negative side: exp(-x) overflows, expit is 0
    w_ref = R.np_weights(Ax)
    assert 0.35 * n < (w_ref == 0).sum() < 0.65 * n
    X = krcn.DeviceCSR(A)
    w = X.weights(t(Ax, torch.float64))
    assert np.array_equal(h(w) == 0, w_ref == 0)
    v = rng.standard_normal(d)
    for l2 in (0.0, 0.01):
        e = rel_err(h(X.hvp(w, t(v, torch.float64), l2=l2)), O.hvp_from_weights(A, w_ref, v, l2))
        print(f"hvp with {int((w_ref == 0).sum())} of {n} weights zero, l2 {l2}: rel err {e:.3e}")
        assert e < 1e-13
    X.close()
