"""High-precision reference of the logistic scalar layer, and the error metric
the edge tests share (tests/test_logistic_reference.py on the CPU,
tests/test_gpu_logistic_edges.py on the device).

Exact functions: mpmath at 300 bits of a float input, in forms that do not
cancel (never log(1 + exp(-x)): 1 + exp(-708) is 1 at 300 bits).  Inputs are
floats, so an fp32 grid is converted exactly.

Working-precision formulas: the reference's own operations (loss.py:161-176,
220, 225, 296-297) in numpy at the grid's dtype; their distance from the exact
values is the yardstick a device result is held to.

excess(): the largest error in ulps of a scale, after forgiving one smallest
normal number of absolute error (results below the normal range: a device may
flush where glibc does not).
"""
import math

import mpmath
import numpy as np
from mpmath import mp, mpf

import krcn_oracle as O

PREC = 300      # every computation below runs inside mp.workprec(PREC); the global precision is left alone

SPECIALS = (746, 745.2, 710, 709, 708, 104, 103, 89, 88, 87, 40, 37, 36.8, 36.7, 33, 18, 17, 1)
SEED = 20260


# ------------------------------------------------------------------- exact
def _each(fn, x):
    with mp.workprec(PREC):
        return [fn(mpf(float(v))) for v in np.asarray(x).ravel()]


def _expit(x):
    return 1 / (1 + mpmath.exp(-x))


def _softplus(x):
    """log(1 + exp(x)) without cancellation."""
    return mpmath.log1p(mpmath.exp(x)) if x < 0 else x + mpmath.log1p(mpmath.exp(-x))


def _logsig(x):
    return -mpmath.log1p(mpmath.exp(-x)) if x >= 0 else x - mpmath.log1p(mpmath.exp(x))


def _weight(x):
    e = mpmath.exp(-abs(x))
    return e / (1 + e) ** 2


def exact_expit(x):
    return _each(_expit, x)


def exact_logsig(x):
    return _each(_logsig, x)


def exact_mid_branch(x):
    """x - exp(x): the expression of logsig's branch on [-33, -18), not the function."""
    return _each(lambda v: v - mpmath.exp(v), x)


def exact_weights(x):
    return _each(_weight, x)


def exact_residual(x, b):
    """expit(x) - b for b in {0, 1}; b = 1 as -expit(-x)."""
    if b == 0:
        return exact_expit(x)
    assert b == 1
    return _each(lambda v: -_expit(-v), x)


def exact_loss_term(x, b):
    """(1 - b) x - logsig(x); b = 0 is softplus(x), b = 1 softplus(-x)."""
    if b == 0:
        return _each(_softplus, x)
    if b == 1:
        return _each(lambda v: _softplus(-v), x)
    return _each(lambda v: (1 - mpf(float(b))) * v - _logsig(v), x)


# -------------------------------------------------------------------- grid
def margin_grid(dtype):
    """About 6000 distinct finite margins of `dtype`: every threshold of the
    scalar layer (the logsig branches, where exp over- and underflows in fp64
    and fp32, where expit rounds to 1) with its neighbours, a regular sweep of
    [-50, 50] and 2000 draws of 30 N(0, 1)."""
    dt = np.dtype(dtype)
    pts = []
    for s in SPECIALS + (0,):
        for v in {dt.type(s), dt.type(-s)}:
            pts += [v, np.nextafter(v, dt.type(np.inf)), np.nextafter(v, dt.type(-np.inf))]
    pts = np.array(pts, dtype=dt)
    sweep = np.linspace(-50, 50, 4001).astype(dt)
    draws = (30.0 * np.random.default_rng(SEED).standard_normal(2000)).astype(dt)
    return np.unique(np.concatenate([pts, sweep, draws]))


# ------------------------------------------------------------------ metric
def _bits(dtype):
    return {np.dtype(np.float64): 53, np.dtype(np.float32): 24}[np.dtype(dtype)]


def tiny(dtype):
    with mp.workprec(PREC):
        return mpf(float(np.finfo(dtype).tiny))


def ulp(v, dtype):
    """Spacing of `dtype` at magnitude v >= tiny (an mpf or a float)."""
    with mp.workprec(PREC):
        v = abs(mpf(v))
        _, e = mpmath.frexp(v)          # v = m 2^e, 0.5 <= m < 1
        return mpmath.ldexp(mpf(1), int(e) - _bits(dtype))


def excess(got, exact, dtype, scale=None):
    """max_i (|got_i - exact_i| - tiny) / ulp(max(scale_i, tiny)); scale
    defaults to |exact_i|.  inf when a got_i is not finite."""
    got = np.asarray(got).ravel()
    assert len(got) == len(exact)
    if not np.isfinite(got).all():
        return math.inf
    t = tiny(dtype)
    scale = exact if scale is None else scale
    worst = mpf("-inf")
    with mp.workprec(PREC):
        for g, e, s in zip(got, exact, scale):
            err = (abs(mpf(float(g)) - e) - t) / ulp(max(abs(mpf(s)), t), dtype)
            worst = max(worst, err)
    return float(worst)


def loss_scale(x, exact_terms):
    """max(|a|, |t|): what the term's two operands and its result are rounded at."""
    with mp.workprec(PREC):
        return [max(abs(mpf(float(a))), abs(t)) for a, t in zip(np.asarray(x).ravel(), exact_terms)]


def round_to(v, dtype):
    """An mpf of the normal range rounded to the nearest value of `dtype` (ties to even)."""
    assert abs(v) >= tiny(dtype)
    with mp.workprec(_bits(dtype)):
        r = +v
    return np.dtype(dtype).type(float(r))


def tie_distance(v, dtype):
    """Distance of v from the nearest rounding tie of `dtype`, in ulps of v (0 .. 0.5)."""
    with mp.workprec(PREC):
        q = abs(mpf(v)) / ulp(v, dtype)
        return float(abs(q - mpmath.floor(q) - mpf(0.5)))


# ------------------------------------------- the reference's formulas, numpy
def np_expit(x):
    one = x.dtype.type(1)
    with np.errstate(over="ignore", under="ignore"):
        return one / (one + np.exp(-x))


def np_logsig(x):
    with np.errstate(over="ignore", under="ignore"):
        return O.logsig(x)


def np_weights(x):
    a = np_expit(x)
    with np.errstate(under="ignore"):
        return a * (x.dtype.type(1) - a)


def np_residual(x, b):
    return np_expit(x) - x.dtype.type(b)


def np_loss_term(x, b):
    b = np.full_like(x, b)
    with np.errstate(over="ignore", under="ignore"):
        return (x.dtype.type(1) - b) * x - np_logsig(x)


# ---------------------------------------------- the four compared quantities
def reference_excesses(dtype):
    """{name: excess of the numpy formula on margin_grid(dtype)} with the exact
    values and scales the device tests reuse: (grid, {name: (np_excess, exact, scale)})."""
    x = margin_grid(dtype)
    ex_s = exact_expit(x)
    out = {}

    def put(name, got, exact, scale=None):
        out[name] = (excess(got, exact, dtype, scale), exact, scale)

    put("expit", np_expit(x), ex_s)
    put("logsig", np_logsig(x), exact_logsig(x))
    put("weights", np_weights(x), exact_weights(x), ex_s)
    put("residual_b1", np_residual(x, 1), exact_residual(x, 1), [mpf(1)] * len(x))
    for b in (0, 1):
        t = exact_loss_term(x, b)
        put(f"loss_b{b}", np_loss_term(x, b), t, loss_scale(x, t))
    return x, out
