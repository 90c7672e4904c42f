"""Generate tests/golden/f9_dense_values32.npz by running the REFERENCE on the
problem of f8_dense.npz with every matrix value rounded to fp32 and widened
back (A32 = double(float(A))): what a dense pass with fp32 value storage
(KRCN_VALUES_F32) on an fp64 handle computes with.

Run where the reference is checked out, with its directory given:
    python tests/golden/make_golden_dense_values32.py PATH_TO_REFERENCE
(or KRCN_REFERENCE=PATH_TO_REFERENCE in the environment).

The reference is imported from its own directory with the stubs of
make_golden_dense.py: `numba.njit` replaced by the identity and no bytecode
written.  The output is plain data: the problem and what the reference
returned; no reference source is copied.

Problem: krcn.synth.make_dense_problem(130, 75, 0.97, seed=31) with
data.astype(float32).astype(float64) (no value of that problem is
fp32-exact); x, the three v, the l2 set, Lanczos m in {10, 20} and the 8-step
Cubic_Krylov_LS run are those of f8, and so are the keys.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import scipy.sparse as sp

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("KRCN_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "optimizer")):
    sys.exit("usage: make_golden_dense_values32.py PATH_TO_REFERENCE (the directory that holds optimizer/loss.py)")
REF = os.path.abspath(REF)

numba_stub = types.ModuleType("numba")
numba_stub.njit = lambda f=None, **kw: f if f is not None else (lambda g: g)
sys.modules["numba"] = numba_stub
sys.path.insert(0, REF)
from optimizer.cubic import Cubic_Krylov_LS, Lanczos  # noqa: E402  (the reference's)
from optimizer.loss import LogisticRegression  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
from krcn import synth  # noqa: E402  (pure-numpy generator, no device code)

assert sys.modules["optimizer.loss"].__file__.startswith(REF)

N, D, FILL, SEED = 130, 75, 0.97, 31
L2S = (0.0, 0.01)


def main():
    A64, b = synth.make_dense_problem(N, D, FILL, seed=SEED)
    data = A64.data.astype(np.float32).astype(np.float64)
    assert not np.any(data == A64.data)
    A = sp.csr_matrix((data, A64.indices.copy(), A64.indptr.copy()), shape=A64.shape)
    x = np.random.default_rng(11).uniform(-0.3, 0.3, size=D)
    rv = np.random.default_rng(12)
    vs = [rv.standard_normal(D) for _ in range(3)]
    out = dict(shape=np.array(A.shape), indptr=A.indptr, indices=A.indices, data=A.data, b=b, x=x,
               fill=np.array(FILL), seed=np.array(SEED), l2s=np.array(L2S))
    for k, v in enumerate(vs):
        out[f"v{k}"] = v
    for t, l2 in enumerate(L2S):
        loss = LogisticRegression(A, b, l1=0, l2=l2, store_mat_vec_prod=True)
        if t == 0:
            out["b01"] = np.asarray(loss.b, dtype=np.float64)
        out[f"Ax_l2_{t}"] = np.array(loss.mat_vec_product(x), copy=True)
        out[f"value_l2_{t}"] = np.array(loss.value(x))
        out[f"grad_l2_{t}"] = np.array(loss.gradient(x), copy=True)
        for k, v in enumerate(vs):
            out[f"hvp{k}_l2_{t}"] = np.array(loss.hess_vec_prod(x, v), copy=True)
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    g = loss.gradient(x)
    out["g"] = np.array(g, copy=True)
    for m in (10, 20):
        V, al, be, beta = Lanczos(lambda q: loss.hess_vec_prod(x, q), g, m=m)
        out[f"V_m{m}"], out[f"alphas_m{m}"], out[f"betas_m{m}"], out[f"beta_m{m}"] = V, al, be, np.array(beta)
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    opt = Cubic_Krylov_LS(loss=loss, reg_coef=1e-3, label="krylov", subspace_dim=10, tolerance=1e-9, tqdm=False)
    opt.run(x0=np.full(D, 0.5), it_max=8)
    opt.compute_loss_of_iterates()
    tr = opt.trace
    out.update(crn_xs=np.asarray(tr.xs), crn_its=np.asarray(tr.its), crn_solver_its=np.asarray(tr.solver_its),
               crn_loss_vals=np.asarray(tr.loss_vals), crn_final_reg_coef=np.array(opt.reg_coef),
               crn_final_value=np.array(opt.value))
    np.savez_compressed(os.path.join(HERE, "f9_dense_values32.npz"), **out)
    print("f9_dense_values32.npz:", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
