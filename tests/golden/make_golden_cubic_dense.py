"""Generate tests/golden/f10_cubic_dense.npz by running the REFERENCE's
cubic_solver_root (optimizer/cubic.py:40-75, dense branch) on dense blocks.

Run where the reference is checked out, with its directory given:
    python tests/golden/make_golden_cubic_dense.py PATH_TO_REFERENCE
(or KRCN_REFERENCE=PATH_TO_REFERENCE in the environment).

The reference is imported from its own directory with the stubs of
make_golden.py (`numba.njit` replaced by the identity, no bytecode written).
The output is plain data: inputs and what the reference returned.

Layout: matrices H_<i> / vectors g_<i>, and per case c the arrays hidx[c] (which
H / g), M[c], eps[c], r0[c], group[c] (0, 1, 2 below), raises[c], its[c],
lam[c], dec[c], cond[c] (group 1: cond_2(H + lam I), else 0) and s_<c>.

  group 0  partial Hessians of the f6 problem (synth seed 5, 3,000 x 400,
           30,000 nonzeros, l2 = 0) at x = 0.5: the reference's
           partial_gradient / partial_hessian over
           default_rng(31).choice(400, k, replace=False) for
           k in {1, 2, 10, 63, 64, 65, 100, 128}; M in {5e-4, 1e-2, 1},
           eps in {machine epsilon, 1e-8}, r0 = 0.1.
  group 1  ill-conditioned blocks H = B^T diag(w) B / 500, symmetrised, with
           B = N(500, 4) N(4, k) + noise N(500, k), w ~ U(0.05, 0.25),
           g = 1e-3 N(k) (default_rng(32), drawn in that order per block);
           noise in {1e-2, 1e-4}, k in {16, 48}, M in {1e-6, 1e-2}, both eps.
  group 2  one indefinite block (k = 8, an eigenvalue of -1 < -r0): the
           reference raises LinAlgError; inputs and the flag only.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("KRCN_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "optimizer")):
    sys.exit("usage: make_golden_cubic_dense.py PATH_TO_REFERENCE (the directory that holds optimizer/cubic.py)")
REF = os.path.abspath(REF)

numba_stub = types.ModuleType("numba")
numba_stub.njit = lambda f=None, **kw: f if f is not None else (lambda g: g)
sys.modules["numba"] = numba_stub
sys.path.insert(0, REF)
from optimizer.loss import LogisticRegression  # noqa: E402  (the reference's)
from optimizer.cubic import cubic_solver_root  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
from krcn import synth  # noqa: E402  (pure-numpy generator, no device code)

assert sys.modules["optimizer.cubic"].__file__.startswith(REF)

EPS = float(np.finfo(float).eps)
KS_A = (1, 2, 10, 63, 64, 65, 100, 128)
MS_A = (5e-4, 1e-2, 1.0)


def main():
    out, cases = {}, []
    mats = 0

    def add_matrix(H, g):
        nonlocal mats
        out[f"H_{mats}"], out[f"g_{mats}"] = np.ascontiguousarray(H), np.ascontiguousarray(g)
        mats += 1
        return mats - 1

    def add_case(hidx, M, eps, group):
        H, g = out[f"H_{hidx}"], out[f"g_{hidx}"]
        c = dict(hidx=hidx, M=M, eps=eps, r0=0.1, group=group, raises=0, its=0, lam=0.0, dec=0.0, cond=0.0)
        try:
            s, its, lam, dec = cubic_solver_root(g, H, M, epsilon=eps, r0=0.1)
            c.update(its=int(its), lam=float(lam), dec=float(dec))
            if group == 1:
                c["cond"] = float(np.linalg.cond(H + lam * np.eye(len(g)), 2))
        except np.linalg.LinAlgError:
            c["raises"] = 1
            s = np.zeros(len(g))
        out[f"s_{len(cases)}"] = np.asarray(s, dtype=np.float64)
        cases.append(c)

    # group 0
    A, b = synth.make_problem(None, seed=5, n=3000, d=400, nnz=30_000)
    loss = LogisticRegression(A.tocsc(), b, l1=0, l2=0, store_mat_vec_prod=True)
    x = np.full(A.shape[1], 0.5)
    rng = np.random.default_rng(31)
    for k in KS_A:
        I = rng.choice(A.shape[1], size=k, replace=False)
        g = np.asarray(loss.partial_gradient(x, I)).ravel()
        H = np.asarray(loss.partial_hessian(x, I).toarray())
        h = add_matrix(H, g)
        out[f"I_{h}"] = I.astype(np.int32)
        for M in MS_A:
            for eps in (EPS, 1e-8):
                add_case(h, M, eps, 0)
    # group 1
    rng = np.random.default_rng(32)
    for noise in (1e-2, 1e-4):
        for k in (16, 48):
            B = rng.standard_normal((500, 4)) @ rng.standard_normal((4, k)) + noise * rng.standard_normal((500, k))
            w = rng.uniform(0.05, 0.25, size=500)
            H = B.T @ (w[:, None] * B) / 500
            H = (H + H.T) / 2
            g = 1e-3 * rng.standard_normal(k)
            h = add_matrix(H, g)
            for M in (1e-6, 1e-2):
                for eps in (EPS, 1e-8):
                    add_case(h, M, eps, 1)
    # group 2
    rng = np.random.default_rng(33)
    Q, _ = np.linalg.qr(rng.standard_normal((8, 8)))
    H = Q @ np.diag([-1.0, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]) @ Q.T
    H = (H + H.T) / 2
    h = add_matrix(H, rng.standard_normal(8))
    add_case(h, 1e-2, 1e-8, 2)
    assert cases[-1]["raises"] == 1 and not any(c["raises"] for c in cases[:-1])

    for key in ("hidx", "group", "raises", "its"):
        out[key] = np.array([c[key] for c in cases], dtype=np.int64)
    for key in ("M", "eps", "r0", "lam", "dec", "cond"):
        out[key] = np.array([c[key] for c in cases], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "f10_cubic_dense.npz"), **out)
    print("f10_cubic_dense.npz:", len(cases), "cases,", mats, "matrices; cond range of group 1:",
          min(c["cond"] for c in cases if c["group"] == 1), max(c["cond"] for c in cases if c["group"] == 1))
    print("its:", [c["its"] for c in cases])


if __name__ == "__main__":
    main()
