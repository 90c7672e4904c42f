"""The reference of krcn_cgs2 (oracle/krcn_oracle.py: cgs2_apply) pinned on the
CPU, and the bound (cgs2_bound) at which tests/test_gpu_cgs2.py compares the
device sweeps with it, checked on the reference alone.

The shapes and inputs are built here and imported by the GPU file, so both see
one set.  Inputs of every case: V entries N(0, 1) / sqrt(d) (rows near unit
length but far from orthogonal, so each of the two passes changes z at O(1) and
neither hides the other), z entries N(0, 1), default_rng([d, k]), rounded to
the dtype before either side sees them.

What is asserted:
  - cgs2_apply is exact rational arithmetic (fractions.Fraction) on d = 7,
    k = 3, to 16 units of the longdouble's last place on the scales S1 / S2,
    and the float32 variant rounds z1 and z2 where the kernels store them
    (to the nearest float32 of the exact values);
  - the bound is not too tight: a plain float64 numpy evaluation that sums in
    another order (BLAS products over a fixed permutation of the columns and
    the reversed rows) stays inside it at every shape, on z2 and on ||z2||^2;
  - the bound is sharp enough: at every shape with k >= 2, each of three
    float64 evaluations with one fault exceeds it by at least 1e4 in some
    component: pass 2 skips row k - 1; pass 2 forms its dots with column
    c + 1's value in place of column c's, for one c; pass 1 skips the last
    256-row range (rows 256 ((k - 1) // 256) and up).
A shape with d = 1 has no column c + 1 and k = 1 no second row: the faults are
asserted at the other 77 of the 81 shapes.
Measured over the shapes below: the reordered evaluation reaches at most 0.023
of the bound on z2 (d = 1; 2.6e-6 at the least: the bound grows with d + k, the
error of a pairwise sum hardly) and 0.033 on ||z2||^2; the faults exceed it by
3.1e5 (skipped row, d = 131,073), 1.8e6 (wrong column) and 8.4e5 (skipped
range) at the least.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import krcn_oracle as O

NPDT = {"fp64": np.float64, "fp32": np.float32}
E = {"fp64": 2, "fp32": 4}                      # elements of a 16-byte vector

# ---- the batched sweeps (krcn_cgs2.hpp: k_cgs_rowdots .. k_cgs_update_norm)
# every d here is odd with d % 4 != 0 (rows of neither dtype are whole 16-byte vectors) but 32 and 64, where
# the GPU file forces these sweeps with a z that starts one element into its buffer
ROW_EDGES_K = (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 2043)
ROW_EDGES_D = 33
COL_EDGES_D = (1, 31, 32, 33, 63, 64, 65)
COL_EDGES_K = 17
# cgs_rd_chunks(d, k) = max(1, min(1024 // k, d // 4096)):
#   (8191, 300) min(3, 1) = 1    (8193, 300) min(3, 2) = 2    (12289, 341) min(3, 3) = 3
#   (12289, 342) min(2, 3) = 2   (8193, 513) min(1, 2) = 1
CHUNK_CASES = {(8191, 300): 1, (8193, 300): 2, (12289, 341): 3, (12289, 342): 2, (8193, 513): 1}
COEFF_ROUNDS_CASE = (65_569, 17)                # ceil(d / 32) = 2050 slabs: a second round of 2048 in k_cgs_coeffs
NORM_STRIDE_CASE = (131_073, 9)                 # ceil(d / 64) = 2049 > kMaxPartials = 2048 blocks: one block takes two slabs
BATCHED = sorted({(ROW_EDGES_D, k) for k in ROW_EDGES_K} | {(d, COL_EDGES_K) for d in COL_EDGES_D}
                 | set(CHUNK_CASES) | {COEFF_ROUNDS_CASE, NORM_STRIDE_CASE})

# ---- the 1 KiB-piece sweeps (k_cgs_rowdots_v, k_cgs_colsweep); d in units of E
PIECE_UNROLL_K = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)
PIECE_RANGE_K = (256, 257, 513, 1792, 1793, 2043)          # Q = 1, 2, 3, 7, 8, 8 ranges of 256 rows
PIECE_GROUPS_NV = (1, 63, 64, 65)                          # d = E, 64 E - E, 64 E, 64 E + E
PIECE_GROUPS_K = 33
# chunks of a row of nv vectors: S = cgs_rdv_steps(nv) doubles from 1 while S * 256 * 16 < nv (cap 16),
# C = cgs_rdv_chunks(nv, S) = ceil(nv / (256 S)):
#   nv = 256 -> S 1, C 1      1793 -> S 1, C 8      2049 -> S 1, C 9      3841 -> S 1, C 16
#   4097 -> S 2, C 9          65537 -> S 16, C 17 (past kCgsRdChunksV = 16)
PIECE_CHUNKS_NV = {256: (1, 1), 1793: (1, 8), 2049: (1, 9), 3841: (1, 16), 4097: (2, 9), 65_537: (16, 17)}
PIECE_CHUNKS_K = 5
PIECE = sorted({(65, k) for k in PIECE_UNROLL_K + PIECE_RANGE_K} | {(nv, PIECE_GROUPS_K) for nv in PIECE_GROUPS_NV}
               | {(nv, PIECE_CHUNKS_K) for nv in PIECE_CHUNKS_NV})


def rdv_steps_chunks(nv):
    """cgs_rdv_steps / cgs_rdv_chunks of krcn_cgs2.hpp."""
    s = 1
    while s < 16 and s * 256 * 16 < nv:
        s *= 2
    return s, -(-nv // (256 * s))


def rd_chunks(d, k):
    """cgs_rd_chunks of krcn_cgs2.hpp."""
    return max(1, min(1024 // k, d // 4096))


def all_shapes():
    """Every (d, k) a GPU case runs: the batched ones as listed, the 1 KiB-piece ones for both vector widths."""
    return sorted(set(BATCHED) | {(nv * e, k) for nv, k in PIECE for e in E.values()})


@functools.lru_cache(maxsize=None)
def inputs(d, k, prec):
    """(V, z) of a case in the dtype; read-only."""
    rng = np.random.default_rng([d, k])
    V = (rng.standard_normal((k, d)) / np.sqrt(d)).astype(NPDT[prec])
    z = rng.standard_normal(d).astype(NPDT[prec])
    V.setflags(write=False)
    z.setflags(write=False)
    return V, z


@functools.lru_cache(maxsize=4)
def reference(d, k, prec):
    """(z1, z2, norm2, bound, norm2_bound) of a case; read-only."""
    V, z = inputs(d, k, prec)
    z1, z2, n2, S1, S2 = O.cgs2_apply(V, z, NPDT[prec])
    bound, n2_bound = O.cgs2_bound(V, z1, z2, S1, S2, NPDT[prec])
    for a in (z1, z2, bound):
        a.setflags(write=False)
    return z1, z2, n2, bound, n2_bound


def ratio(z2_got, z2_ref, bound):
    """Largest component error in units of the bound."""
    err = np.abs(np.asarray(z2_got).astype(np.longdouble) - z2_ref).astype(np.float64)
    return float((err / bound).max())


# ------------------------------------------------------------------ exactness
def exact_cgs2(V, z):
    Vf = [[Fraction(float(x)) for x in row] for row in V]
    zf = [Fraction(float(x)) for x in z]

    def sweep(y):
        h = [sum(a * b for a, b in zip(row, y)) for row in Vf]
        return [yc - sum(Vf[r][c] * h[r] for r in range(len(Vf))) for c, yc in enumerate(y)]

    z1 = sweep(zf)
    return z1, sweep(z1)


def frac(x):
    """A longdouble as an exact Fraction (its float64 head and tail are both exact)."""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))


def nearest32(fr):
    """The float32 nearest to a Fraction, found among the neighbours of the float64 quotient's rounding."""
    c = np.float32(fr.numerator / fr.denominator)
    cands = (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)))
    return min(cands, key=lambda v: abs(Fraction(float(v)) - fr))


ULP64 = Fraction(1, 2 ** 63)    # of a longdouble's 64-bit significand, relative


def test_cgs2_apply_is_exact_on_a_tiny_case():
    """Every longdouble operation errs by at most 2^-64 relative, and a component of z1 or z2 is the end of
    2 (k + 1) + 2 of them on the scale S1 (S2): within 16 units of 2^-63 of that scale of the exact value,
    2,000 times below a float64's own rounding."""
    V, z = inputs(7, 3, "fp64")
    z1e, z2e = exact_cgs2(V, z)
    z1, z2, n2, S1, S2 = O.cgs2_apply(V, z)
    Va = np.abs(V)
    np.testing.assert_allclose(S1, np.abs(z) + Va.T @ (Va @ np.abs(z)), rtol=1e-15)
    z1d = np.abs(np.asarray(z1, dtype=np.float64))
    np.testing.assert_allclose(S2, z1d + Va.T @ (Va @ z1d), rtol=1e-15)
    for c in range(7):
        assert abs(frac(z1[c]) - z1e[c]) <= 16 * ULP64 * Fraction(float(S1[c]))
        # z2 is formed from the longdouble z1, whose own error pass 2 carries on the scale S2
        assert abs(frac(z2[c]) - z2e[c]) <= 16 * ULP64 * Fraction(float(S2[c] + Va[:, c] @ (Va @ S1) + S1[c]))
    n2e = sum(frac(x) ** 2 for x in z2)
    assert abs(frac(n2) - n2e) <= 16 * ULP64 * n2e
    # the passes matter at O(1) on these inputs: neither z1 nor z2 is z to rounding
    assert np.abs(np.asarray(z1 - z, dtype=np.float64)).max() > 0.1
    assert np.abs(np.asarray(z2 - z1, dtype=np.float64)).max() > 0.01


def test_cgs2_apply_float32_rounds_where_the_kernels_store():
    V, z = inputs(7, 3, "fp32")
    z1e, _ = exact_cgs2(V, z)
    z1, z2, n2, _, _ = O.cgs2_apply(V, z, np.float32)
    z1r = [nearest32(fr) for fr in z1e]
    assert [np.float32(x) for x in z1] == z1r and all(float(np.float32(x)) == float(x) for x in z1)
    # z2 is formed from the ROUNDED z1, exactly, then rounded
    Vf = [[Fraction(float(x)) for x in row] for row in V]
    y = [Fraction(float(x)) for x in z1r]
    h = [sum(a * b for a, b in zip(row, y)) for row in Vf]
    z2e = [yc - sum(Vf[r][c] * h[r] for r in range(3)) for c, yc in enumerate(y)]
    assert [np.float32(x) for x in z2] == [nearest32(fr) for fr in z2e]
    assert all(float(np.float32(x)) == float(x) for x in z2)
    n2e = sum(Fraction(float(x)) ** 2 for x in z2)
    assert abs(frac(n2) - n2e) <= 16 * ULP64 * n2e


# ---------------------------------------------------- the bound, both ways
def float64_cgs2(V, z, perm=None, skip_row2=None, wrong_col=None, skip_from1=None):
    """z2 and ||z2||^2 by plain float64 numpy.  perm: the columns in that order
    and the rows reversed (another summation order).  Faults: pass 2 without
    row skip_row2; pass 2's dots with column wrong_col + 1's value of V in place
    of column wrong_col's; pass 1 without the rows from skip_from1 on."""
    V = np.asarray(V, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    if perm is not None:
        inv = np.argsort(perm)
        Vp = np.ascontiguousarray(V[::-1, perm])
        z2, n2 = float64_cgs2(Vp, z[perm])
        return z2[inv], n2
    V1 = V[:skip_from1] if skip_from1 is not None else V
    z1 = z - V1.T @ (V1 @ z)
    Vd = V
    if wrong_col is not None:
        Vd = V.copy()
        Vd[:, wrong_col] = V[:, wrong_col + 1]
    h2 = Vd @ z1
    if skip_row2 is not None:
        h2[skip_row2] = 0.0
    z2 = z1 - V.T @ h2
    return z2, float(z2 @ z2)


@pytest.mark.parametrize("d,k", all_shapes(), ids=lambda v: str(v))
def test_bound_holds_for_a_reordered_float64_evaluation_and_catches_faults(d, k):
    V, z = inputs(d, k, "fp64")
    z1, z2, n2, bound, n2_bound = reference(d, k, "fp64")
    assert (bound > 0).all()
    perm = np.random.default_rng(3).permutation(d)
    for p in (None, perm):
        got, gn2 = float64_cgs2(V, z, perm=p)
        r, rn = ratio(got, z2, bound), abs(gn2 - float(n2)) / n2_bound
        print(f"d = {d}, k = {k}, {'reordered' if p is not None else 'plain'}: error / bound {r:.3g}, norm2 {rn:.3g}")
        assert r <= 1.0 and rn <= 1.0
    if k < 2 or d < 2:
        return
    c = int(np.argmax(np.abs(np.asarray(z1, dtype=np.float64))[:-1]))   # a column whose z1 weighs in the dots
    faults = {"pass 2 skips row k - 1": dict(skip_row2=k - 1),
              "pass 2 reads column c + 1 for c": dict(wrong_col=c),
              "pass 1 skips the last row range": dict(skip_from1=256 * ((k - 1) // 256))}
    for name, kw in faults.items():
        r = ratio(float64_cgs2(V, z, **kw)[0], z2, bound)
        print(f"d = {d}, k = {k}, {name}: error / bound {r:.3g}")
        assert r >= 1e4, name
