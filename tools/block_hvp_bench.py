#!/usr/bin/env python3
"""Block HVP against k single HVPs on one handle (run by hand on the GPU).

For every synthetic shape (default news20 rcv1 w8a, fp64) one resident process
builds the problem and the handle, builds the handle's automatic pass plans,
warms both paths up and then, for every k (default 2 4 8 16), times in
alternation, `--alternations` times each, by device events:

  block    `--reps` krcn_hvp_block calls over a (d, k) block with one shared w
  singles  `--reps` times k back-to-back DeviceCSR.hvp calls, one per column,
           under the handle's AUTO plans (the code of the parent commit)

Reported per shape and k: us per block and per vector (medians over the
alternations, with every alternation's figures), the ratio block / singles per
alternation, whether the block was the faster in all of them, and the achieved
fraction of 8 TB/s on the algorithmic bytes of a block HVP,
2 * (idx + val) * nnz + 2 * 4 * (n + d + 2) + 8 k (2 d + 2 n) + 8 n (w)
(both CSRs streamed once, V read, U written and read, Y written).
The largest relative difference between the block's columns and the singles'
results is recorded too (summation orders differ: expected around 1e-15).

--hessian N D NNZ also times LogisticRegression.hessian(x, block=16) against
hessian(x) on a synthetic N x D problem (D > KRCN_COORD_MAX), host clock around
a device synchronise, one run each after a warm-up.

    python tools/block_hvp_bench.py [--shapes news20 rcv1] [--ks 8 16] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))


def block_hvp_bytes(n, d, nnz, k, s_val=8, s_idx=4, s_ptr=4):
    matrix = 2 * (s_idx + s_val) * nnz + 2 * s_ptr * (n + d + 2)
    return matrix + s_val * k * (2 * d + 2 * n) + s_val * n


def bench_shape(shape, ks, alternations, reps):
    import numpy as np
    import torch

    import krcn
    from krcn import synth

    A, _ = synth.make_problem(shape)
    n, d = A.shape
    X = krcn.DeviceCSR(A)
    fmt = X.plan_format()    # builds the AUTO plans (with their placement probe) before anything is timed
    g = torch.Generator(device="cpu").manual_seed(1)
    w = (0.05 + 0.2 * torch.rand(n, generator=g, dtype=torch.float64)).to(X.device)
    rows = []
    for k in ks:
        V = torch.randn((d, k), generator=g, dtype=torch.float64).to(X.device)
        cols = [V[:, j].contiguous() for j in range(k)]
        outs = [X.empty_d() for _ in range(k)]
        Y = torch.empty((d, k), dtype=torch.float64, device=X.device)

        def block():
            X.hvp_block(w, V, out=Y)

        def singles():
            for c, o in zip(cols, outs):
                X.hvp(w, c, out=o)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return 1e3 * e0.elapsed_time(e1) / reps

        for _ in range(3):
            block()
            singles()
        torch.cuda.synchronize()
        ref = torch.stack(outs, dim=1)
        diff = float((Y - ref).abs().max() / ref.abs().max())
        tb, ts = [], []
        for _ in range(alternations):
            tb.append(timed(block))
            ts.append(timed(singles))
        ratios = [b / s for b, s in zip(tb, ts)]
        us = statistics.median(tb)
        nbytes = block_hvp_bytes(n, d, A.nnz, k)
        rows.append({"shape": shape, "n": n, "d": d, "nnz": int(A.nnz), "k": k, "plans": fmt,
                     "block_us": round(us, 2), "block_us_per_vector": round(us / k, 2),
                     "singles_us": round(statistics.median(ts), 2),
                     "singles_us_per_vector": round(statistics.median(ts) / k, 2),
                     "block_us_all": [round(x, 2) for x in tb], "singles_us_all": [round(x, 2) for x in ts],
                     "block_over_singles": [round(r, 4) for r in ratios],
                     "block_faster_in_all": all(r < 1.0 for r in ratios),
                     "algorithmic_mb": round(nbytes / 1e6, 1),
                     "fraction_of_8_TBps": round(nbytes / (us * 1e-6) / 8e12, 4),
                     "max_rel_diff_vs_singles": diff})
        print(json.dumps(rows[-1]), flush=True)
    X.close()
    return rows


def bench_hessian(n, d, nnz):
    import numpy as np
    import torch

    from krcn import synth
    from optimizer.loss import LogisticRegression

    A, b = synth.make_problem(None, seed=1, n=n, d=d, nnz=nnz)
    loss = LogisticRegression(A, b, l2=0.01, store_mat_vec_prod=True)
    x = np.full(d, 0.05)

    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        H = loss.hessian(x, **kw)
        torch.cuda.synchronize()
        return H, time.perf_counter() - t0

    timed(block=16)
    H0, t0 = timed()
    H16, t16 = timed(block=16)
    r = {"hessian": {"n": n, "d": d, "nnz": int(A.nnz), "columns_s": round(t0, 4), "block16_s": round(t16, 4),
                     "block16_over_columns": round(t16 / t0, 4),
                     "max_rel_diff": float(np.abs(H16 - H0).max() / np.abs(H0).max())}}
    print(json.dumps(r), flush=True)
    return r["hessian"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["news20", "rcv1", "w8a"])
    ap.add_argument("--ks", nargs="+", type=int, default=[2, 4, 8, 16])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hessian", nargs=3, type=int, default=None, metavar=("N", "D", "NNZ"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("block_hvp_bench.py needs an MI355X: it measures, it does not fall back")
    result = {"alternations": args.alternations, "reps": args.reps, "cases": []}
    for shape in args.shapes:
        result["cases"] += bench_shape(shape, args.ks, args.alternations, args.reps)
    if args.hessian:
        result["hessian"] = bench_hessian(*args.hessian)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
