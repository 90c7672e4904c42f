"""The dense plan format's ABI surface and its geometry rule (krcn_dense_geometry
is host arithmetic: no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "krcn.h")

SHAPES = [(1, 1), (1, 7), (9, 1), (3, 130), (130, 3), (67, 129), (300, 257), (44, 7129), (6000, 5000),
          (200_000, 2_000_000)]
DTYPES = [(0, 8), (1, 4)]   # (KRCN_F64, bytes), (KRCN_F32, bytes)


def geometry(rows, cols, dtype, lanes=0, slicing=0):
    from krcn import _lib
    out = (ctypes.c_int64 * 8)()
    _lib.call("krcn_dense_geometry", rows, cols, dtype, lanes, slicing, out)
    keys = ("ld", "L", "S", "width", "groups", "grid", "bytes", "nvec")
    return dict(zip(keys, (int(v) for v in out)))


def test_header_declares_the_dense_format():
    text = open(HEADER).read()
    assert re.search(r"\bKRCN_FORMAT_DENSE\s*=\s*5\b", text)
    assert re.search(r"\bKRCN_PLAN_DENSE\s*=\s*6\b", text)
    assert re.search(r"krcn_status\s+krcn_dense_geometry\s*\(", text)


def test_binding_matches_the_header():
    from krcn import _lib
    text = open(HEADER).read()
    for name in ("KRCN_FORMAT_DENSE", "KRCN_PLAN_DENSE", "KRCN_PLAN_JAG"):
        assert getattr(_lib, name) == int(re.search(rf"\b{name}\s*=\s*(\d+)", text).group(1))
    assert "krcn_dense_geometry" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "krcn_dense_geometry")


@pytest.mark.parametrize("dtype,vs", DTYPES)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_geometry_invariants(rows, cols, dtype, vs):
    vw = 16 // vs
    for lanes in (0, 2, 8, 64):
        for slicing in (0, 1, 8, 64):
            g = geometry(rows, cols, dtype, lanes, slicing)
            assert g["ld"] >= cols and (g["ld"] * vs) % 16 == 0
            assert g["nvec"] == -(-cols // vw) and g["ld"] == g["nvec"] * vw
            assert g["width"] % vw == 0 and g["width"] >= vw          # whole vectors, at least one
            assert g["S"] >= 1 and g["S"] * g["width"] >= cols
            assert g["S"] <= g["nvec"]                                 # every slice keeps a vector
            assert g["L"] in (1, 2, 4, 8, 16, 32, 64)
            if lanes:
                assert g["L"] == lanes
            if slicing == 1:
                assert g["S"] == 1
            if slicing >= 8:
                assert g["S"] == min(slicing, g["nvec"])
            rows_per_group = 256 // g["L"]
            assert g["groups"] == -(-rows // rows_per_group)
            assert g["grid"] % g["S"] == 0 and 1 <= g["grid"] // g["S"] <= g["groups"]
            assert g["bytes"] == rows * g["ld"] * vs                   # exact: no 32-bit or 64-bit wrap


@pytest.mark.parametrize("dtype,vs", DTYPES)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_sequential_policy_is_one_lane_one_slice(rows, cols, dtype, vs):
    for slicing in (0, 1, 8):
        g = geometry(rows, cols, dtype, lanes=1, slicing=slicing)
        assert g["L"] == 1 and g["S"] == 1 and g["width"] == g["ld"]


@pytest.mark.parametrize("dtype,vs", DTYPES)
def test_forced_slices_clamp_to_the_vectors(dtype, vs):
    g = geometry(5, 3, dtype, lanes=0, slicing=8)
    assert g["nvec"] == -(-3 * vs // 16)
    assert g["S"] == g["nvec"] and g["S"] < 8
    assert g["S"] * g["width"] >= 3


@pytest.mark.parametrize("dtype,vs", DTYPES)
def test_bytes_at_the_largest_shape_do_not_overflow(dtype, vs):
    g = geometry(200_000, 2_000_000, dtype)
    assert g["bytes"] == 200_000 * 2_000_000 * vs > 2 ** 40
    gt = geometry(2_000_000, 200_000, dtype)
    assert gt["bytes"] == g["bytes"]
    # the largest shape the int32 indices address saturates instead of wrapping
    top = geometry(2 ** 31 - 1, 2 ** 31 - 1, dtype)
    assert 0 < top["bytes"] <= 2 ** 63 - 1 and top["bytes"] >= (2 ** 31 - 1) ** 2


def test_auto_slices_a_pass_with_few_long_rows():
    """duke's pass 1 (44 rows of 7,129) cannot fill the CUs with rows alone; gisette's passes can."""
    duke = geometry(44, 7129, 0)
    assert duke["S"] > 1 and duke["grid"] > 44 // 4
    assert (duke["nvec"] // duke["S"]) * 16 >= 4096                     # a slice keeps >= 4 KiB of a row
    for rows, cols in ((6000, 5000), (5000, 6000)):
        assert geometry(rows, cols, 0)["S"] == 1
        assert geometry(rows, cols, 1)["S"] == 1


def test_bad_arguments_are_invalid():
    from krcn import _lib
    lib = _lib.load()
    out = (ctypes.c_int64 * 8)()
    assert lib.krcn_dense_geometry(4, 4, 0, 0, 0, None) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_dense_geometry(-1, 4, 0, 0, 0, out) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_dense_geometry(4, 4, 2, 0, 0, out) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_dense_geometry(4, 4, 0, 3, 0, out) == _lib.KRCN_ERR_INVALID
    assert lib.krcn_dense_geometry(4, 4, 0, 0, 12, out) == _lib.KRCN_ERR_INVALID


def test_make_dense_problem_is_deterministic_and_exact():
    from krcn import synth
    A, b = synth.make_dense_problem(37, 45, 0.7, seed=5)
    A2, b2 = synth.make_dense_problem(37, 45, 0.7, seed=5)
    assert A.shape == (37, 45) and A.indices.dtype == np.int32 and A.indptr.dtype == np.int32
    np.testing.assert_array_equal(A.indptr, A2.indptr)
    np.testing.assert_array_equal(A.indices, A2.indices)
    np.testing.assert_array_equal(A.data, A2.data)
    np.testing.assert_array_equal(b, b2)
    assert set(np.unique(b)) <= {-1.0, 1.0}
    assert A.has_sorted_indices and np.all(A.data != 0.0) and np.abs(A.data).max() <= 1.0
    dense = A.toarray()
    assert np.count_nonzero(dense) == A.nnz and 0.55 < A.nnz / dense.size < 0.85
    full, _ = synth.make_dense_problem(20, 30, 1.0, seed=5)
    assert full.nnz == 600
