"""Host sanitizer runs of the library's multithreaded host code (SURVEY.md §5,
"Race detection"; the GPU side has no sanitizer on this pool).

`make asan` / `make tsan` (krylov-cubic-regularized-newton_amd/csrc/Makefile)
build, with g++ and AddressSanitizer + UBSan or ThreadSanitizer:
  * rendezvous_{asan,tsan}: the virtual communicator's rendezvous
    (csrc/krcn_rendezvous.hpp, the code krcn_comm_create_virtual runs) driven
    by 2, 3, 8 and 16 threads through thousands of all-reduces with a host
    sum, plus its two failure paths (a rank that never arrives, a rank that
    passes another count);
  * svm_cli_{asan,tsan}: the multithreaded svmlight parser (csrc/
    krcn_svmlight.hip) behind a command line; the inputs of
    tests/test_libsvm.py go through it and must equal sklearn's parse;
  * layout_asan: the pass-plan layouts (csrc/krcn_layout.hpp) behind
    tests/native/layout_check.cpp, which checks every layout's invariants on
    small patterns at the boundaries of the layout rules (ASan + UBSan only:
    the layouts are single-threaded);
  * lzstep_asan: the Lanczos step choice (csrc/krcn_lzstep.hpp) behind
    tests/native/lzstep_check.cpp; tests/test_lanczos_step.py runs it.
A sanitizer finding aborts the program (-fno-sanitize-recover), so every
check here is also "no report".
"""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "csrc")
NATIVE = os.path.join(REPO, "krylov-cubic-regularized-newton_amd", "lib", "native")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module", autouse=True)
def built():
    r = subprocess.run(["make", "-C", CSRC, "asan", "tsan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_rendezvous_stress(san):
    r = subprocess.run([os.path.join(NATIVE, f"rendezvous_{san}"), "1500"], capture_output=True, text=True,
                       env=ENV, timeout=300)
    assert r.returncode == 0 and "rendezvous stress ok" in r.stdout, r.stdout + r.stderr[-4000:]
    assert "WARNING" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-4000:]


def _cli(san, path, threads, tmp_path):
    out = tmp_path / f"out_{san}_{threads}.bin"
    r = subprocess.run([os.path.join(NATIVE, f"svm_cli_{san}"), str(path), str(threads), str(out)],
                       capture_output=True, text=True, env=ENV, timeout=300)
    assert "WARNING" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    if r.returncode == 2:
        return r.stderr.strip()
    assert r.returncode == 0, r.stderr[-4000:]
    raw = out.read_bytes()
    rows, nnz, _, _ = np.frombuffer(raw[:32], dtype=np.int64)
    o = 32
    indptr = np.frombuffer(raw[o:o + 8 * (rows + 1)], dtype=np.int64); o += 8 * (rows + 1)
    indices = np.frombuffer(raw[o:o + 8 * nnz], dtype=np.int64); o += 8 * nnz
    data = np.frombuffer(raw[o:o + 8 * nnz], dtype=np.float64); o += 8 * nnz
    labels = np.frombuffer(raw[o:o + 8 * rows], dtype=np.float64)
    return indptr, indices, data, labels


def _same_as_sklearn(san, path, threads, tmp_path):
    from sklearn.datasets import load_svmlight_file
    indptr, indices, data, labels = _cli(san, path, threads, tmp_path)
    A, b = load_svmlight_file(str(path), zero_based=True)   # unshifted, as the parser reports them
    np.testing.assert_array_equal(indptr, A.indptr)
    np.testing.assert_array_equal(indices, A.indices)
    assert data.tobytes() == A.data.tobytes()
    assert labels.tobytes() == np.asarray(b, dtype=np.float64).tobytes()


GRAMMAR = ("# header comment\n"
           "+1 qid:7 1:0.5 3:2e0 10:-1.5E-3   # trailing comment\r\n"
           "\n"
           "   -1\t2:.25 4:+7. 5:1e-320\n"
           "0.5\n"
           "-1 1:inf 2:-Infinity 3:nan 6:123456789.123456789123\n"
           "  # only a comment\n"
           "2 7:1e308 8:1e400 9:-1e-400")


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_svm_grammar(san, tmp_path):
    p = tmp_path / "g.svm"
    p.write_bytes(GRAMMAR.encode())
    _same_as_sklearn(san, p, 1, tmp_path)


@pytest.mark.parametrize("san", ["asan", "tsan"])
@pytest.mark.parametrize("line,msg", [
    ("1 3:1 2:1", "sorted and unique"),
    ("1 2:1 2:1", "sorted and unique"),
    ("1 -2:1", "Invalid index"),
    ("1 2:abc", "could not convert"),
    ("abc 2:1", "could not convert"),
    ("1 x:1", "invalid literal"),
])
def test_svm_errors(san, line, msg, tmp_path):
    p = tmp_path / "bad.svm"
    p.write_text("1 1:1\n" + line + "\n")
    err = _cli(san, p, 1, tmp_path)
    assert isinstance(err, str) and msg in err


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_svm_multithreaded_large_file(san, tmp_path):
    """A 2+ MB file cut into byte ranges for 1, 8 and 13 threads: sklearn's
    arrays every time, and no sanitizer report from the threaded parse or the
    threaded stitch."""
    from sklearn.datasets import dump_svmlight_file
    from krcn import synth
    A, b = synth.make_problem(None, seed=11, n=4000, d=50_000, nnz=300_000)
    path = tmp_path / "big.svm"
    dump_svmlight_file(A, b, str(path), zero_based=False)
    assert path.stat().st_size > (2 << 20)
    for t in (1, 8, 13):
        _same_as_sklearn(san, path, t, tmp_path)


# ---------------------------------------------------------------- plan layouts
# layout_asan (tests/native/layout_check.cpp): the host-only pass-plan layouts
# of csrc/krcn_layout.hpp on small patterns at the boundaries of their rules.
# The program checks every layout invariant itself (cuts, caps, partitions,
# flags, task tables) and exits non-zero on a violation or a sanitizer report;
# the tests add what the boundary should decide.
from test_plan_layouts import run_layout, write_pattern   # noqa: E402

LAYOUT = os.path.join(NATIVE, "layout_asan")
WAVE, SORTED, WINDOW, JAG = 1, 2, 3, 4
KW = {"f64": 16352, "f32": 36800}        # WinGeom<T>::kW = (163,840 - 16 slabs of 256 values - 256) / sizeof(T)
KW1 = {"f64": 20448, "f32": 40896}       # JagGeom<T>::kW1 (one window)
KW2 = {"f64": 9200, "f32": 19424}        # JagGeom<T>::kW2 (two windows beside the product slabs)


def _pattern(tmp_path, lengths, cols, seed=0, name="p.bin"):
    """Rows of the given lengths over `cols` columns (sorted, unique), as layout_check reads them."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    idx = [np.sort(rng.choice(cols, size=int(n), replace=False)) for n in lengths if n]
    path = tmp_path / name
    write_pattern(path, np.concatenate([[0], np.cumsum(lengths)]), np.concatenate(idx) if idx else [], cols)
    return path


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 129])
def test_layout_row_counts(rows, dt, tmp_path):
    """Every format around the 64-row group / tile edge; no rows at all: the jagged format refuses."""
    p = _pattern(tmp_path, [3] * rows, 500)
    for fmt in (WAVE, SORTED, WINDOW, JAG):
        for pass_ in (1, 2):
            got = run_layout(LAYOUT, p, fmt, dt, pass_, expect_refusal=fmt == JAG and rows == 0)
            if fmt == JAG and rows == 0:
                assert "empty or too narrow" in got["refused"]
            elif fmt == JAG:
                assert got["ntiles"] == (rows + 63) // 64 and got["grid"] >= 1
            else:
                assert got["grid"] >= 1


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_layout_empty_rows_and_no_nonzeros(dt, tmp_path):
    """Empty rows at the start, in the middle and at the end; a matrix without nonzeros."""
    lengths = [0] * 70 + [5, 9, 2] * 30 + [0] * 130 + [7] * 40 + [0] * 66
    p = _pattern(tmp_path, lengths, 3000)
    z = _pattern(tmp_path, [0] * 100, 3000, name="z.bin")
    for fmt in (WAVE, SORTED, WINDOW, JAG):
        for slicing in ((0, 8) if fmt in (WAVE, SORTED) else (0,)):
            run_layout(LAYOUT, p, fmt, dt, 1, slicing=slicing)
            got = run_layout(LAYOUT, z, fmt, dt, 1, slicing=slicing, expect_refusal=fmt == JAG)
            assert ("refused" in got) == (fmt == JAG)


def test_layout_jag_long_row_thresholds(tmp_path):
    """kJagLong: a row of 32 elements stays in the lane-per-row units, one of 33 goes long.  With a
    window that leaves fewer than 256 task partials (20,400 fp64 entries: 48), rows go long only once
    some row passes the 254 elements an 8-bit lane count holds."""
    for n, nlong in ((32, 0), (33, 1)):
        got = run_layout(LAYOUT, _pattern(tmp_path, [4] * 100 + [n] + [4] * 100, 500), JAG, "f64", 1)
        assert (got["S"], got["lthr"], got["nlong"]) == (1, 32, nlong)
    for n, lthr, nlong in ((254, 0, 0), (255, 32, 2)):
        got = run_layout(LAYOUT, _pattern(tmp_path, [4] * 100 + [n, 40] + [4] * 100, 20_400), JAG, "f64", 1)
        assert (got["S"], got["tcap"], got["lthr"], got["nlong"]) == (1, 48, lthr, nlong)
    # the sequential lane policy keeps every row lane-per-row
    got = run_layout(LAYOUT, _pattern(tmp_path, [4] * 100 + [33] + [4] * 100, 500), JAG, "f64", 1, seq=1)
    assert got["nlong"] == 0


def test_layout_jag_task_cap(tmp_path):
    """One block (64 rows) whose long row needs tcap - 1, tcap and tcap + 1 tasks of 128 elements
    (tcap = 48 beside a 20,400-entry fp64 window): the last is refused."""
    for tasks in (47, 48):
        got = run_layout(LAYOUT, _pattern(tmp_path, [4] * 30 + [128 * tasks] + [4] * 33, 20_400), JAG, "f64", 1)
        assert (got["grid"], got["tcap"], got["nlong"], got["maxtasks"]) == (1, 48, 1, tasks)
    got = run_layout(LAYOUT, _pattern(tmp_path, [4] * 30 + [128 * 49] + [4] * 33, 20_400), JAG, "f64", 1,
                     expect_refusal=True)
    assert "long rows need 49 tasks (max 48)" in got["refused"]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_layout_window_and_jag_slice_edges(dt, tmp_path):
    """One more column than a window holds: the jagged format leaves its single window at kW1 for
    ceil(cols / kW2) = 3 double-buffered slices; the forced window format goes from 4 accumulate slices
    to window slices at 4 kW."""
    lengths = [3] * 200
    assert run_layout(LAYOUT, _pattern(tmp_path, lengths, KW1[dt]), JAG, dt, 1)["S"] == 1
    assert run_layout(LAYOUT, _pattern(tmp_path, lengths, KW1[dt] + 1), JAG, dt, 1)["S"] == -(-(KW1[dt] + 1) // KW2[dt]) == 3
    got = run_layout(LAYOUT, _pattern(tmp_path, lengths, 4 * KW[dt]), WINDOW, dt, 1)
    assert (got["kind"], got["S"], got["W"]) == (4, 4, KW[dt])
    got = run_layout(LAYOUT, _pattern(tmp_path, lengths, 4 * KW[dt] + 1), WINDOW, dt, 1)
    assert (got["kind"], got["S"], got["grid"]) == (3, 8, 256)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_layout_xt_copy_edge(dt, tmp_path):
    """The per-block X^T copy of a one-piece accumulate plan: made up to 1,024 columns, not past them."""
    lengths = [4] * 300 + [0] * 20 + [900] + [4] * 100
    assert run_layout(LAYOUT, _pattern(tmp_path, lengths, 1024), WINDOW, dt, 1, accum=1)["xt"] == 1
    assert run_layout(LAYOUT, _pattern(tmp_path, lengths, 1025), WINDOW, dt, 1, accum=1)["xt"] == 0


def test_layout_window_slices_empty_chunks(tmp_path):
    """Fewer tiles (300 rows: at most 19) than the 32 blocks of each of 8 slices: blocks with an empty
    row chunk still name their slice."""
    got = run_layout(LAYOUT, _pattern(tmp_path, [40] * 300, 100_000), WINDOW, "f64", 1)
    assert (got["kind"], got["S"], got["kpb"], got["grid"]) == (3, 8, 32, 256)
    assert got["ntiles"] < 32 and got["empty"] >= 8 * (32 - got["ntiles"])


def test_layout_skew_lane_rule(tmp_path):
    """Sorted pass 1, automatic lanes.  Uniform rows of 64: the plain mean's L = 8.  199 rows of 8 and one
    of 4,000: mean 28 (L = 2), nonzero-weighted mean 2,863 >= 2 x 28, so lanes come from 4 x 2,863: 64.
    Pass 2 keeps the plain mean."""
    uni = _pattern(tmp_path, [64] * 200, 5000, name="u.bin")
    skew = _pattern(tmp_path, [8] * 199 + [4000], 5000, name="s.bin")
    assert run_layout(LAYOUT, uni, SORTED, "f64", 1)["L"] == 8
    assert run_layout(LAYOUT, skew, SORTED, "f64", 1)["L"] == 64
    assert run_layout(LAYOUT, skew, SORTED, "f64", 2)["L"] == 2
