"""The tiles of window-slices plans on the host (CPU).

tests/native/win_tiles_check.cpp runs csrc/krcn_layout.hpp's win_layout over
inputs of its own (empty row runs, an empty slice, rows past a chunk, tiles of
exactly 256 slots from a misaligned start, a row count that is no multiple of
64, skewed rows, the 85 x 3 block mapping, both sides of the rule's threshold)
and checks the tiling's invariants; built with g++ under ASan + UBSan and run
as a program of its own.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "csrc")
EXE = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "lib", "native", "win_tiles_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_win_tiles_invariants():
    r = subprocess.run(["make", "-C", CSRC, "win_tiles"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, env=ENV, timeout=300)
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    got = {ln.split(":")[0]: dict(kv.split("=") for kv in ln.split(": ", 1)[1].split()) for ln in lines[:-1]}
    # the data-cut tilings fill their chunks; the fixed tiling of the same matrix does not
    assert got["uniform+edges"]["datacut"] == "1" and float(got["85x3"]["fill"]) > 0.95
    assert float(got["uniform+edges forced R=32"]["fill"]) < 0.7
    assert got["short stream"]["datacut"] == "0" and got["row-capped"]["R"] == "64"
