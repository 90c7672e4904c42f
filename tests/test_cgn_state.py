"""The state rule of krcn_cubic_cg (csrc/krcn_cgn_state.hpp), on the CPU.

tests/native/cgn_state_check.cpp (built with ASan + UBSan by `make cgn_state`, a
stand-alone program) drives the rule the way the kernels do — tick by tick,
every kernel of a tick restated as a loop — over a diagonal H, where the "CG
solve" is the exact elementwise division, and prints what each chain leaves.
Here every case is rerun through scipy.optimize.root_scalar(method="newton",
x0=r0, xtol=eps, maxiter=it_max) with the host path's phi and phi'
(optimizer/cubic.py Cubic_LS.cubic_solver_root_CG):
  equal iteration counts;
  lam within 4 ulp (Python's ** 2 against the rule's product);
  solves = 2 its + 1, or 2 its + 2 when newton() left on phi == 0.
"""
import math
import os
import subprocess
import warnings

import numpy as np
import pytest
from scipy.optimize import root_scalar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "csrc")
EXE = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "lib", "native", "cgn_state_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

H5 = [0.5, 1.25, 2.0, 3.5, 0.75]
G5 = [0.3, -0.2, 0.45, 0.1, -0.6]
# name -> (h, g, M, r0, eps, it_max), as in cgn_state_check.cpp
CASES = {
    "well": (H5, G5, 1.0, 0.1, 1e-8, 100),
    "smallM": (H5, G5, 5e-4, 0.1, 1e-8, 100),
    "itmax1": (H5, G5, 1.0, 0.1, 1e-8, 1),
    "itmax3": (H5, G5, 1.0, 0.1, 1e-8, 3),
    "gzero": (H5, [0.0] * 5, 1.0, 0.1, 1e-8, 100),
    "phizero": ([0.0], [1.0], 1.0, 1.0, 1e-8, 100),
    "notpd": ([0.5, -2.0, 2.0], [0.0, 1.0, 0.0], 1.0, 0.1, 1e-8, 100),
    "nan": (H5, [0.3, math.nan, 0.45, 0.1, -0.6], 1.0, 0.1, 1e-8, 100),
}


@pytest.fixture(scope="module")
def got():
    r = subprocess.run(["make", "-C", CSRC, "cgn_state"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, env=ENV, timeout=60)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"cases={len(CASES)} bad=0"
    out = {}
    for ln in lines:
        if ln.startswith("case "):
            f = ln.split()
            out[f[1]] = dict(kv.split("=") for kv in f[2:])
    assert sorted(out) == sorted(CASES)
    return out


def seq_sum(v):
    t = 0.0
    for x in v:
        t += x
    return t


def host_newton(h, g, M, r0, eps, it_max):
    """The host path's root_scalar call over the diagonal H; also how newton() left."""
    left_on_zero = []

    def y(lam):
        return [gi / (hi + lam) for hi, gi in zip(h, g)]

    def func(lam):
        v = lam ** 2 - M ** 2 * math.sqrt(seq_sum(t * t for t in y(lam))) ** 2
        left_on_zero.append(v == 0.0)
        return v

    def grad(lam):
        yy = y(lam)
        zz = [yi / (hi + lam) for hi, yi in zip(h, yy)]
        return 2 * lam - M ** 2 * (-2 * seq_sum(a * b for a, b in zip(yy, zz)))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol = root_scalar(func, fprime=grad, x0=r0, method="newton", maxiter=it_max, xtol=eps)
    return sol, left_on_zero[-1]


def ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


@pytest.mark.parametrize("name", ["well", "smallM", "itmax1", "itmax3", "phizero"])
def test_chain_matches_root_scalar(got, name):
    h, g, M, r0, eps, it_max = CASES[name]
    sol, on_zero = host_newton(h, g, M, r0, eps, it_max)
    r = got[name]
    its = int(r["its"])
    assert its == sol.iterations
    assert ulps(float.fromhex(r["lam"]), sol.root) <= 4
    assert int(r["status"]) == (0 if sol.converged else 3)
    assert int(r["solves"]) == 2 * its + (2 if on_zero else 1)
    assert int(r["cg_iterations"]) == int(r["solves"])      # one exact "iteration" per solve
    assert int(r["s_zero"]) == 0
    # the closing expressions on s = -(H + lam I)^{-1} g
    lam = float.fromhex(r["lam"])
    y = [gi / (hi + lam) for hi, gi in zip(h, g)]
    ns = math.sqrt(seq_sum(t * t for t in y))
    assert float.fromhex(r["ns"]) == ns
    dec = lam / 2 * (ns * ns) - M / 3 * (ns * ns * ns) - (-seq_sum(gi * yi for gi, yi in zip(g, y))) / 2
    assert float.fromhex(r["dec"]) == dec


def test_statuses_of_the_cases(got):
    assert got["well"]["status"] == "0" and got["smallM"]["status"] == "0"
    assert got["itmax1"]["status"] == "3" and got["itmax1"]["its"] == "1" and got["itmax1"]["solves"] == "3"
    assert got["itmax3"]["status"] == "3" and got["itmax3"]["its"] == "3"
    assert got["phizero"]["its"] == "0" and got["phizero"]["solves"] == "2"
    assert float.fromhex(got["phizero"]["lam"]) == 1.0


def test_zero_gradient_is_the_halving_sequence(got):
    """g = 0: every solve has a zero right-hand side (no CG iteration), phi = lam^2,
    phi' = 2 lam: the rule's three expressions, evaluated here, exactly."""
    h, g, M, r0, eps, it_max = CASES["gzero"]
    p0, its = r0, 0
    M2 = M * M
    for itr in range(it_max):
        fval = p0 * p0 - M2 * (0.0 * 0.0)
        fder = 2.0 * p0 - M2 * (-2.0 * 0.0)
        p = p0 - fval / fder
        its = itr + 1
        if p == p0 or abs(p - p0) <= eps:
            break
        p0 = p
    r = got["gzero"]
    assert int(r["its"]) == its and float.fromhex(r["lam"]) == p
    assert r["status"] == "0" and r["cg_iterations"] == "0" and r["s_zero"] == "1"
    assert int(r["solves"]) == 2 * its + 1
    assert int(r["ticks"]) == int(r["solves"])               # a zero right-hand side takes one tick
    sol, _ = host_newton(h, g, M, r0, eps, it_max)
    assert sol.iterations == its and ulps(sol.root, p) <= 4


def test_an_indefinite_operator_is_status_1(got):
    r = got["notpd"]            # p = g = e_2, (h_2 + r0) = -1.9: p.q < 0 in the first iteration
    assert r["status"] == "1" and r["its"] == "0" and r["solves"] == "1" and r["s_zero"] == "1"
    assert r["ticks"] == "2"    # the failing tick and the one that zeroes s


def test_a_nan_in_g_is_status_4(got):
    r = got["nan"]
    assert r["status"] == "4" and r["its"] == "0" and r["solves"] == "0" and r["s_zero"] == "1"
    assert r["cg_iterations"] == "0" and r["ticks"] == "1"
