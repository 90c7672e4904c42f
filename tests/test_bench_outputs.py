"""bench.py --dump-outputs: what dump_outputs writes for a Lanczos result, on
CPU tensors (whole V when small, the fixed seeded sample above the limit, rows
past m_eff as zeros, the same files from the same arguments), and the
argument checks of a plain run."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(m, d, m_eff, dtype):
    g = torch.Generator().manual_seed(5)
    V = torch.randn((m, d), generator=g, dtype=torch.float64).to(dtype)
    al = np.arange(1.0, m_eff + 1.0)
    be = np.arange(1.0, m_eff) / 7.0
    return V, al, be, types.SimpleNamespace(m_eff=m_eff)


def test_small_basis_is_dumped_whole(tmp_path):
    V, al, be, info = _result(6, 37, 4, torch.float32)
    bench.dump_outputs(str(tmp_path / "o"), V, al, be, info)
    assert sorted(os.listdir(tmp_path / "o")) == ["V.npy", "alphas.npy", "betas.npy"]
    got = np.load(tmp_path / "o" / "V.npy")
    assert got.dtype == np.float32 and got.shape == (6 * 37,)
    want = V.numpy().copy()
    want[4:] = 0   # rows >= m_eff are not part of the basis
    assert np.array_equal(got.reshape(6, 37), want)
    a, b = np.load(tmp_path / "o" / "alphas.npy"), np.load(tmp_path / "o" / "betas.npy")
    assert a.dtype == b.dtype == np.float64
    assert np.array_equal(a, al) and np.array_equal(b, be)


def test_large_basis_is_sampled_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_V_ELEMS", 1000)
    V, al, be, info = _result(9, 501, 7, torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), V, al, be, info)
    bench.dump_outputs(str(tmp_path / "b"), V.clone(), al, be, info)
    got = np.load(tmp_path / "a" / "V_sample.npy")
    assert got.dtype == np.float64 and got.shape == (1000,)
    assert np.array_equal(got, np.load(tmp_path / "b" / "V_sample.npy"))
    idx = np.sort(np.random.default_rng(20240117).integers(0, 9 * 501, 1000, dtype=np.int64))
    want = V.numpy().reshape(-1)[idx].copy()
    want[idx // 501 >= 7] = 0
    assert np.array_equal(got, want)
    assert (idx // 501 >= 7).any() and np.count_nonzero(got) > 500


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--steps must be >= 1" in r.stderr
    assert '"metric"' not in r.stdout
