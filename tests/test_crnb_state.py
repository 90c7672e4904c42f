"""The per-column state rule of the batched Krylov-CRN step (csrc/krcn_crnb_state.hpp), on the CPU.

tests/native/crnb_state_check.cpp (built with ASan + UBSan by `make crnb_state`,
a stand-alone program) walks every sequence of trial outcomes for max_trials <= 4
— R: the trial is rejected, A: accepted, N: value_new is a NaN (the reference's
`while` condition is false: accepted), F / G: the solve fails with status 1 / 2 —
through a restatement of cubic.py:293-303 and through the rule the way the
kernels drive it (max_trials + 1 trials enqueued, a column that has ended skipped),
and compares what each leaves.  The expected lines below are recomputed here
from the reference's loop, by hand:
  the chain ends at the first outcome that is not R, or after max_trials + 1 R's;
  trials  = the R's before that point (max_trials at the cap);
  solves  = trials + 1;
  M       = reg_coef * beta / beta ** trials;
  end     = accepted (A, N), failed (F, G), capped.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "csrc")
EXE = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "lib", "native", "crnb_state_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
REG, BETA = 1e-3, 0.5


@pytest.fixture(scope="module")
def lines():
    r = subprocess.run(["make", "-C", CSRC, "crnb_state"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, env=ENV, timeout=60)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def expected(max_trials, seq):
    first = next((i for i, ch in enumerate(seq) if ch != "R"), None)
    if first is None:
        end, trials = "capped", max_trials
    else:
        end, trials = {"A": "accepted", "N": "accepted", "F": "failed", "G": "failed"}[seq[first]], first
    M = REG * BETA
    for _ in range(trials):
        M = M / BETA
    return dict(end=end, trials=trials, solves=trials + 1, M=M)


def test_every_sequence_matches_the_reference(lines):
    rules = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in lines if ln.startswith("rule ")]
    assert len(rules) == sum(5 ** (mt + 1) for mt in range(5)) == 3905
    assert lines[-1] == "cases=3910 bad=0"
    for got in rules:
        mt, seq = int(got["max"]), got["seq"]
        assert len(seq) == mt + 1
        e = expected(mt, seq)
        assert got["end"] == e["end"], got
        assert int(got["trials"]) == e["trials"], got
        assert int(got["solves"]) == e["solves"], got
        assert float.fromhex(got["M"]) == e["M"], got


def test_the_cases_by_hand(lines):
    by = {(ln.split()[1], ln.split()[2]): ln for ln in lines if ln.startswith("rule ")}
    # accepted at once: M = reg * beta, no backtracking
    assert by[("max=2", "seq=ARR")].endswith(f"end=accepted trials=0 solves=1 M={(REG * BETA).hex()}")
    # two rejections, then accepted: the later trials are no-ops
    assert by[("max=4", "seq=RRARR")].endswith(f"end=accepted trials=2 solves=3 M={(REG * BETA / BETA / BETA).hex()}")
    # the cap: max_trials rejections and one more failing trial end the chain, M is the last solve's
    assert by[("max=2", "seq=RRR")].endswith(f"end=capped trials=2 solves=3 M={(REG * BETA / BETA / BETA).hex()}")
    assert by[("max=0", "seq=R")].endswith(f"end=capped trials=0 solves=1 M={(REG * BETA).hex()}")
    # a failing solve ends the column with the M it was given
    assert by[("max=3", "seq=RFAA")].endswith(f"end=failed trials=1 solves=2 M={(REG * BETA / BETA).hex()}")
    # a NaN value fails the `>` test: accepted, as the reference's while
    assert by[("max=1", "seq=NR")].endswith("end=accepted trials=0 solves=1 M=" + (REG * BETA).hex())


def test_inactive_columns_run_nothing(lines):
    inactive = [ln for ln in lines if ln.startswith("inactive ")]
    assert len(inactive) == 5
    for ln in inactive:
        assert f"end=inactive trials=0 solves=0 M={(REG * BETA).hex()}" in ln
