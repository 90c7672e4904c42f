"""How a window-slices block's waves share its tiles, on the host (CPU).

tests/native/win_claim_check.cpp replays win_stream's protocol — a static deal
of each wave's first ring fill, then claims from one counter per block — for 16
simulated waves over csrc/krcn_geom.hpp's claim arithmetic, under many orders
of drawing the counter (one wave taking every claim, round-robin, one slow
wave, seeded random orders), for segment lengths at every edge of the deal, and
checks that every tile is run exactly once and none outside the segment; built
with g++ under ASan + UBSan and run as a program of its own.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "csrc")
EXE = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "lib", "native", "win_claim_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_win_claim_invariants():
    r = subprocess.run(["make", "-C", CSRC, "win_claim"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, env=ENV, timeout=300)
    print(r.stdout)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    # both run lengths, every length and first tile, 3 + 4 + 200 orders each
    assert [ln.split(":")[0] for ln in lines[:-1]] == ["run 1", "run 3"]
    for ln in lines[:-1]:
        got = dict(kv.split("=") for kv in ln.split(": ", 1)[1].split())
        assert got == {"lengths": "13", "firsts": "3", "orders": str(13 * 3 * 207)}
