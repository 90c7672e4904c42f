"""krcn.vec.VecContext (krcn_lz_ext_step, krcn_vec_dot, krcn_vec_div,
krcn_vec_axpy) called directly, fp64 and fp32, at lengths around a wave, a
block and the 1024-block grid cap (where the grid-stride loops take further
trips) and at length 0.

dot and lz_step run on small integers, so every product and sum is exact in
either dtype and in any order: the results are compared bitwise with Python
integers.  div and axpy are compared bitwise with numpy's IEEE division and
its separately rounded multiply and add (the build's -ffp-contract=off: a
fused multiply-add would round once).
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from krcn.vec import VecContext

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 256 * 1024
L = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, CAP - 1, CAP, CAP + 1, CAP + 257, 3 * CAP + 1]
DTYPES = {"fp64": (np.float64, torch.float64), "fp32": (np.float32, torch.float32)}


@pytest.fixture(scope="module")
def vctx():
    c = VecContext(DEV)
    yield c
    c.close()


@pytest.fixture(params=list(DTYPES), ids=list(DTYPES))
def dt(request):
    return DTYPES[request.param]


def dev(a, tdt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, tdt)


def host(x):
    return x.detach().cpu().numpy()


def ints(rng, n):
    return rng.integers(-3, 4, n)


# ---------------------------------------------------------------------- dot
def test_dot_is_the_integer_sum(vctx, dt):
    npdt, tdt = dt
    rng = np.random.default_rng(23)
    for n in L:
        a, b = ints(rng, n), ints(rng, n)
        if n:
            a[-1], b[-1] = -3, 3
        got = vctx.dot(dev(a.astype(npdt), tdt), dev(b.astype(npdt), tdt))
        assert got == float(int((a * b).sum())), f"n = {n}"
    assert vctx.dot(torch.empty(0, dtype=tdt, device=DEV), torch.empty(0, dtype=tdt, device=DEV)) == 0.0


def test_a_short_reduction_after_a_long_one(vctx, dt):
    """One context, the longest vector (1024 partials) and then a short one
    (one partial): the longer call's partials stay out of the shorter sum."""
    npdt, tdt = dt
    rng = np.random.default_rng(29)
    for n in (L[-1], 5, CAP + 257, 65, 1):
        a, b = ints(rng, n), ints(rng, n)
        a[:] = np.where(a == 0, 2, a)
        b[:] = np.where(b == 0, -1, b)
        ad, bd = dev(a.astype(npdt), tdt), dev(b.astype(npdt), tdt)
        assert vctx.dot(ad, bd) == float(int((a * b).sum())), f"n = {n}"
        z = torch.empty_like(ad)
        alpha, nrm = vctx.lz_step(ad, bd, None, 0.0, z)
        al = int((a * b).sum())
        if abs(al) <= 4096:
            assert alpha == float(al) and nrm == math.sqrt(int(((a - al * b) ** 2).sum())), f"n = {n}"
        else:
            assert alpha == float(al), f"n = {n}"


# ---------------------------------------------------------------------- div
def test_div_is_ieee_division(vctx, dt):
    npdt, tdt = dt
    rng = np.random.default_rng(31)
    div = 0.3                 # not an fp32 value: the ABI takes a double and rounds it to the vectors' dtype
    assert float(np.float32(div)) != div
    for n in L:
        a = rng.standard_normal(n).astype(npdt)
        ad = dev(a, tdt)
        keep = ad.clone()
        want = a / npdt(div)
        out = vctx.div(ad, div)
        assert out.dtype == tdt and (n == 0 or out.data_ptr() != ad.data_ptr()) and torch.equal(ad, keep)
        assert np.array_equal(host(out), want), f"n = {n}"
        same = vctx.div(ad, div, out=ad)         # in place, as v = w / beta may be
        assert same.data_ptr() == ad.data_ptr()
        assert np.array_equal(host(ad), want), f"n = {n} in place"
    if npdt == np.float32:
        # the divisor is rounded first: dividing by the double and rounding the quotient gives other bits
        a = rng.standard_normal(4096).astype(np.float32)
        by_double = (a.astype(np.float64) / div).astype(np.float32)
        by_float = a / np.float32(div)
        assert (by_double != by_float).any()
        assert np.array_equal(host(vctx.div(dev(a, tdt), div)), by_float)


# --------------------------------------------------------------------- axpy
def test_axpy_rounds_twice(vctx, dt):
    npdt, tdt = dt
    rng = np.random.default_rng(37)
    alpha = 1.0 / 3.0
    for n in L:
        x = rng.standard_normal(n).astype(npdt)
        y = rng.standard_normal(n).astype(npdt)
        want = y + npdt(alpha) * x
        xd, yd = dev(x, tdt), dev(y, tdt)
        out = vctx.axpy(alpha, xd, yd)
        assert np.array_equal(host(out), want), f"n = {n}"
        assert np.array_equal(host(xd), x) and np.array_equal(host(yd), y)
        same = vctx.axpy(alpha, xd, yd, out=yd)
        assert same.data_ptr() == yd.data_ptr()
        assert np.array_equal(host(yd), want), f"n = {n}, out is y"
    # the data tells the two roundings from one: a fused multiply-add would differ somewhere
    x = rng.standard_normal(4096).astype(npdt)
    y = rng.standard_normal(4096).astype(npdt)
    two = y + npdt(alpha) * x
    al = Fraction(float(npdt(alpha)))
    fused = np.array([float(Fraction(float(yi)) + al * Fraction(float(xi))) for xi, yi in zip(x, y)]).astype(npdt)
    assert (fused != two).any()
    assert np.array_equal(host(vctx.axpy(alpha, dev(x, tdt), dev(y, tdt))), two)


# ------------------------------------------------------------------ lz_step
def lz_case(rng, n):
    """Integer y, v, v_pre in [-3, 3] with |v.(y - 2 v_pre)| <= 4096 and |v.y| <= 4096."""
    y, vp = ints(rng, n), ints(rng, n)
    while True:
        v = ints(rng, n)
        if n:
            v[-1] = 3 if v[-1] >= 0 else -3
        if abs(int((v * (y - 2 * vp)).sum())) <= 4096 and abs(int((v * y).sum())) <= 4096:
            return y, v, vp


@pytest.mark.parametrize("with_pre", [False, True], ids=["step0", "step_j"])
def test_lz_step_on_integers(vctx, dt, with_pre):
    """Every intermediate is an integer below 2^24: alpha = v.w, z = w - alpha v
    and ||z|| are exact in fp32 too.  z is its own buffer, as in
    optimizer.cubic._lanczos_callable (y, v and v_pre are left alone)."""
    npdt, tdt = dt
    rng = np.random.default_rng(41)
    for n in L:
        y, v, vp = lz_case(rng, n)
        w = y - 2 * vp if with_pre else y
        alpha = int((v * w).sum())
        zi = w - alpha * v
        assert n == 0 or np.abs(zi).max() < 2 ** 24
        yd, vd, pd = dev(y.astype(npdt), tdt), dev(v.astype(npdt), tdt), dev(vp.astype(npdt), tdt)
        z = torch.full((n,), 99.0, dtype=tdt, device=DEV)
        got_alpha, got_norm = vctx.lz_step(yd, vd, pd if with_pre else None, 2.0, z)
        assert got_alpha == float(alpha), f"n = {n}"
        assert np.array_equal(host(z), zi.astype(npdt)), f"n = {n}"
        assert got_norm == math.sqrt(int((zi.astype(np.int64) ** 2).sum())), f"n = {n}"
        assert np.array_equal(host(yd), y) and np.array_equal(host(vd), v) and np.array_equal(host(pd), vp)


def test_lz_step_on_random_data(vctx, dt):
    """Against an fp64 restatement at 1e-13 relative (fp32: 1e-5).  y carries 2 v,
    so alpha is O(1) and its relative error means something; the reference sums
    the products with math.fsum."""
    npdt, tdt = dt
    tol = 1e-13 if npdt == np.float64 else 1e-5
    rng = np.random.default_rng(43)
    n = CAP + 257
    v = rng.standard_normal(n)
    v = (v / np.linalg.norm(v)).astype(npdt)
    y = (rng.standard_normal(n) + 2.0 * v).astype(npdt)
    vp = rng.standard_normal(n).astype(npdt)
    beta = 0.37
    z = torch.empty(n, dtype=tdt, device=DEV)
    alpha, nrm = vctx.lz_step(dev(y, tdt), dev(v, tdt), dev(vp, tdt), beta, z)
    y64, v64, p64 = (a.astype(np.float64) for a in (y, v, vp))
    w = y64 - float(npdt(beta)) * p64
    a_ref = math.fsum(v64 * w)
    z_ref = w - a_ref * v64
    n_ref = math.sqrt(math.fsum(z_ref * z_ref))
    assert 1.0 < abs(a_ref) < 4.0
    print(f"alpha {alpha!r} (reference {a_ref!r}, rel {abs(alpha - a_ref) / abs(a_ref):.2e}), "
          f"norm rel {abs(nrm - n_ref) / n_ref:.2e}")
    assert abs(alpha - a_ref) <= tol * abs(a_ref)
    assert np.abs(host(z).astype(np.float64) - z_ref).max() <= tol * np.abs(z_ref).max()
    assert abs(nrm - n_ref) <= tol * n_ref


def test_arguments_are_checked(vctx):
    a = torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        vctx.dot(a, torch.zeros(5, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        vctx.dot(a, torch.zeros(4, dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError):
        vctx.dot(a.to(torch.float16), a.to(torch.float16))
