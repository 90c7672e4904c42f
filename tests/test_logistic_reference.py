"""The high-precision logistic reference (tests/logistic_ref.py) and the
accuracy of the reference's own formulas on the margin grid.

The device tests hold a kernel to "the numpy formula's excess + 2 ulp"; that
only means something while the numpy formulas themselves are accurate on the
grid, so their excess is capped here at 3 ulp per function and dtype (a
condition on the inputs, not a measurement of any kernel).  With glibc 2.35:

    dtype  expit  logsig  weights/expit  residual b=1 (/1)  loss b=0  loss b=1   (loss scaled by max(|a|, |t|))
    fp64   1.73   1.03    2.15           0.72               1.57      0.98
    fp32   2.50   2.03    2.70           0.71               1.76      1.17

Plain relative error of w or of a loss term is not used: w is exactly 0 past
36.7 (fp64) / 16.6 (fp32) and the b = 0 term below -18 cancels to ulp(a), in
the reference as in the port.
"""
import math

import mpmath
import numpy as np
import pytest
import scipy.special
from mpmath import mp, mpf

import logistic_ref as R

DTYPES = [np.float64, np.float32]
CAP = 3.0


@pytest.fixture(scope="module", params=DTYPES, ids=["fp64", "fp32"])
def ref(request):
    x, table = R.reference_excesses(request.param)
    return request.param, x, table


# --------------------------------------------------------------- the helper
@pytest.mark.parametrize("dtype", DTYPES)
def test_grid(dtype):
    x = R.margin_grid(dtype)
    assert x.dtype == np.dtype(dtype) and x.ndim == 1
    assert 5500 <= len(x) <= 6500
    assert np.all(np.diff(x) > 0) and np.isfinite(x).all()
    have = set(x.tolist())
    for s in R.SPECIALS + (0,):
        for v in (dtype(s), dtype(-s)):
            for p in (v, np.nextafter(v, dtype(np.inf)), np.nextafter(v, dtype(-np.inf))):
                assert float(p) in have, p
    assert np.array_equal(x, R.margin_grid(dtype))
    # both sides of every logsig branch
    for th in (-33, -18, 37):
        assert (x < th).any() and (x == th).any()
    assert (x < -50).sum() > 50 and (x > 50).sum() > 50


@pytest.mark.parametrize("dtype", DTYPES)
def test_ulp_is_numpy_spacing(dtype):
    for v in (1.0, 1.5, 2.0, 0.75, 746.0, 1e-30, float(np.finfo(dtype).tiny), 3.0e38):
        assert float(R.ulp(v, dtype)) == float(np.spacing(dtype(v))), v


def test_exact_forms_do_not_cancel():
    """Against the defining expressions at 3000 bits, where they do not cancel either."""
    xs = np.array([-746.0, -709.5, -40.0, -18.0, -0.5, 0.0, 0.5, 18.0, 37.0, 708.5, 746.0])
    got = {"expit": R.exact_expit(xs), "logsig": R.exact_logsig(xs), "w": R.exact_weights(xs),
           "l0": R.exact_loss_term(xs, 0), "l1": R.exact_loss_term(xs, 1), "r1": R.exact_residual(xs, 1)}
    with mp.workprec(3000):
        for i, x in enumerate(xs):
            x = mpf(float(x))
            s = 1 / (1 + mpmath.exp(-x))
            ls = mpmath.log(s)
            want = {"expit": s, "logsig": ls, "w": s * (1 - s), "l0": x - ls, "l1": -ls, "r1": s - 1}
            for k, w in want.items():
                assert abs(got[k][i] - w) <= abs(w) * mpf(2) ** -280, (k, float(x))
    # the form the module avoids: 1 + exp(-708) is 1 at 300 bits
    with mp.workprec(R.PREC):
        assert mpmath.log(1 + mpmath.exp(mpf(-708))) == 0
        assert R.exact_logsig([708.0])[0] < 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_excess_metric(dtype):
    x = np.array([0.3, 1.7, -2.5, 40.0], dtype=dtype)
    exact = R.exact_expit(x)
    rounded = np.array([R.round_to(e, dtype) for e in exact])
    assert R.excess(rounded, exact, dtype) <= 0.5
    off = rounded.copy()
    off[1] = off[1] + 4 * np.spacing(off[1])
    assert 3.5 <= R.excess(off, exact, dtype) <= 4.5
    # a scale: the same absolute error in ulps of 1
    one = [mpf(1)] * len(x)
    assert R.excess(off, exact, dtype, one) < R.excess(off, exact, dtype) + 1e-9
    # below the normal range an absolute error of one smallest normal is forgiven
    small = np.array([0.0], dtype=dtype)
    assert R.excess(small, [R.tiny(dtype) / 3], dtype) <= 0
    assert R.excess(np.array([np.nan], dtype=dtype), [mpf(1)], dtype) == math.inf
    assert R.excess(np.array([np.inf], dtype=dtype), [mpf(1)], dtype) == math.inf


@pytest.mark.parametrize("dtype", DTYPES)
def test_round_to_and_tie_distance(dtype):
    with mp.workprec(R.PREC):
        u = R.ulp(1.0, dtype)
        assert R.round_to(1 + u / 4, dtype) == dtype(1) and R.round_to(1 + 3 * u / 4, dtype) == dtype(1) + dtype(float(u))
        assert R.round_to(1 + u / 2, dtype) == dtype(1)          # tie to even
        assert R.tie_distance(1 + u / 2, dtype) == 0.0
        assert abs(R.tie_distance(1 + u / 4, dtype) - 0.25) < 1e-12
        assert abs(R.tie_distance(mpf(1), dtype) - 0.5) < 1e-12


# ------------------------------------------- the reference's own accuracy
@pytest.mark.parametrize("name", ["expit", "logsig", "weights", "residual_b1", "loss_b0", "loss_b1"])
def test_numpy_formulas_within_3_ulp(ref, name):
    dtype, x, table = ref
    e = table[name][0]
    print(f"{np.dtype(dtype).name} {name}: numpy formula excess {e:.2f} ulp over {len(x)} margins")
    assert e <= CAP


def test_scipy_expit_is_the_naive_form_to_1_ulp_of_1(ref):
    """The oracle calls scipy.special.expit, the kernels 1 / (1 + exp(-x))."""
    dtype, x, _ = ref
    a = scipy.special.expit(x)
    assert a.dtype == np.dtype(dtype)
    dist = np.abs(a.astype(np.float64) - R.np_expit(x).astype(np.float64)).max()
    print(f"{np.dtype(dtype).name}: |scipy expit - naive| max {dist:.3e} (eps {np.finfo(dtype).eps:.3e})")
    assert dist <= np.finfo(dtype).eps


def test_saturation_of_the_numpy_weights(ref):
    """w is exactly 0 where expit rounds to 1 and where exp(-x) overflows; never above 1/4."""
    dtype, x, _ = ref
    w = R.np_weights(x)
    hi, lo = (36.8, -746.0) if dtype == np.float64 else (17.0, -104.0)
    assert (w[x >= hi] == 0).all() and (w[x <= lo] == 0).all()
    assert (w >= 0).all() and (w <= 0.25).all() and w[x == 0][0] == 0.25
