"""How the host cuts the work of the block products (CPU).

tests/native/block_rows_check.cpp runs csrc/krcn_block_rows.hpp over inputs of
its own: the lane group of every k, the short-row grid around every
workgroup's row count and at 2^31 - 1 rows, the long-row list on both sides of
KRCN_BLOCK_LONG_ROW, and a walk of every (workgroup, lane group) and (long row,
segment) the kernels would run, which must own each row and cover each element
exactly once; built with g++ under ASan + UBSan and run as a program of its own.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "csrc")
EXE = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "lib", "native", "block_rows_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_block_rows_invariants():
    r = subprocess.run(["make", "-C", CSRC, "block_rows"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, env=ENV, timeout=300)
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert r.stdout.strip().splitlines() == ["lanes: ok", "grids: ok", "threshold: ok", "cover: ok", "ok"]
