#!/usr/bin/env python3
"""Batched Lanczos against k single Lanczos calls on one handle (run by hand on the GPU).

For every synthetic shape (default w8a rcv1 news20, fp64) one resident process
builds the problem and the handle, builds the handle's automatic pass plans,
warms both paths up (the singles' placement search included) and then, for
every (m, k) — m = 10 everywhere, plus m = 100 on news20; k = 4 8 16 — times in
alternation, `--alternations` times each, by the host clock round the
synchronous calls:

  block    one DeviceCSR.lanczos_block call: k problems over one X, each with
           its own weights (w_cols = k), start vector and l2
  singles  k back-to-back DeviceCSR.lanczos calls, one per problem, on the same
           handle under its AUTO plans (the code of the parent commit)

each repeated `--reps` times per alternation (fewer for the large cases: see
reps_for).  Reported per case: ms per call of either path (medians over the
alternations, with every alternation's figures), us per recurrence step and
problem, the ratio block / singles per alternation, whether the block was the
faster in all of them, and the largest relative difference between the two
paths' alphas and betas (the sums run in different fixed orders: rounding level).

    python tools/lanczos_block_bench.py [--shapes rcv1 w8a] [--ks 8 16] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))


def reps_for(d, k, m, reps):
    """Calls per alternation: `reps`, cut down where one call moves gigabytes."""
    work = d * k * m
    return max(1, min(reps, int(2e9 // max(work, 1)))) if work > 1e8 else reps


def bench_shape(shape, ks, ms, alternations, reps):
    import numpy as np
    import torch

    import krcn
    from krcn import synth

    A, _ = synth.make_problem(shape)
    n, d = A.shape
    X = krcn.DeviceCSR(A)
    fmt = X.plan_format()    # builds the AUTO plans (with their placement probe) before anything is timed
    step = X.lanczos_step()
    gen = torch.Generator(device="cpu").manual_seed(1)
    rows = []
    for m in ms:
        Vs = torch.empty((m, d), dtype=torch.float64, device=X.device)
        for k in ks:
            W = (0.05 + 0.2 * torch.rand((n, k), generator=gen, dtype=torch.float64)).to(X.device)
            G = torch.randn((d, k), generator=gen, dtype=torch.float64).to(X.device)
            l2 = np.array([0.0 if c % 2 else 1e-3 * (c + 1) for c in range(k)])
            wc = [W[:, c].contiguous() for c in range(k)]
            gc = [G[:, c].contiguous() for c in range(k)]
            Vb = torch.empty((m, d, k), dtype=torch.float64, device=X.device)
            nrep = reps_for(d, k, m, reps)

            def block():
                return X.lanczos_block(W, G, m, l2=l2, V=Vb)

            def singles():
                return [X.lanczos(wc[c], gc[c], m, l2=float(l2[c]), V=Vs) for c in range(k)]

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(nrep):
                    fn()
                return 1e3 * (time.perf_counter() - t0) / nrep   # both paths synchronise before they return

            for _ in range(3):   # 3 k >= 12 single calls: past the placement search over the first calls
                b = block()
                s = singles()
            diff = 0.0
            for c in range(k):
                diff = max(diff, float(np.abs(b[1][c] - s[c][1]).max() / np.abs(s[c][1]).max()),
                           float(np.abs(b[2][c] - s[c][2]).max() / np.abs(s[c][2]).max()))
            tb, ts = [], []
            for _ in range(alternations):
                tb.append(timed(block))
                ts.append(timed(singles))
            ratios = [x / y for x, y in zip(tb, ts)]
            mb, msn = statistics.median(tb), statistics.median(ts)
            rows.append({"shape": shape, "n": n, "d": d, "nnz": int(A.nnz), "m": m, "k": k, "plans": fmt,
                         "single_step": step, "reps": nrep,
                         "block_ms": round(mb, 4), "singles_ms": round(msn, 4),
                         "block_us_per_step_and_problem": round(1e3 * mb / (m * k), 2),
                         "singles_us_per_step_and_problem": round(1e3 * msn / (m * k), 2),
                         "block_ms_all": [round(x, 4) for x in tb], "singles_ms_all": [round(x, 4) for x in ts],
                         "block_over_singles": [round(r, 4) for r in ratios],
                         "block_faster_in_all": all(r < 1.0 for r in ratios),
                         "max_rel_diff_vs_singles": diff})
            print(json.dumps(rows[-1]), flush=True)
            del Vb
        del Vs
    X.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["w8a", "rcv1", "news20"])
    ap.add_argument("--ks", nargs="+", type=int, default=[4, 8, 16])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lanczos_block_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("lanczos_block_bench.py needs an MI355X: it measures, it does not fall back")
    result = {"alternations": args.alternations, "reps": args.reps, "cases": []}
    for shape in args.shapes:
        ms = [10, 100] if shape == "news20" else [10]
        result["cases"] += bench_shape(shape, args.ks, ms, args.alternations, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
