#!/usr/bin/env python3
"""The batched Krylov-CRN driver against k single device-step runs (run by hand on the GPU).

For every synthetic shape (default w8a rcv1 news20, fp64, m = 10) one resident
child process — started under its own `timeout -k 10`, the tool stops at the
first child that fails — builds the problem and one LogisticRegression (one
handle, its AUTO plans built before anything is timed), warms both paths up
and then, for every k (4 8 16), times in alternation, `--alternations` times, by
the host clock round the synchronous calls:

  batch    one Cubic_Krylov_LS_Batch.run(x0, it_max) over k columns that differ
           in l2 and reg_coef: one krcn_crn_step_block call per step
  singles  k back-to-back Cubic_Krylov_LS(device_step=True).run(x0, it_max) calls
           of the same problems on the same handle (the code of the parent
           commit; the loss's l2 is set per problem before its run)

Reported per case: ms per step and problem of either path (medians over the
alternations, with every alternation's figures), the ratio batch / singles per
alternation, whether the batch was the faster in all of them, the trials per
step of the batch, and the largest relative difference between the two paths'
final values.

    python tools/crn_step_block_bench.py [--shapes rcv1 w8a] [--ks 8 16] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
M = 10


def columns(k):
    """Per column (l2, reg_coef): every other l2 zero, reg_coef over two decades."""
    return [0.0 if c % 2 else 1e-4 * (c + 1) for c in range(k)], [1e-3 * 10.0 ** ((c % 3) - 1) for c in range(k)]


def bench_shape(shape, ks, alternations, it_max):
    import numpy as np
    import torch

    from krcn import synth
    from optimizer.cubic import Cubic_Krylov_LS, Cubic_Krylov_LS_Batch
    from optimizer.loss import LogisticRegression

    A, b = synth.make_problem(shape)
    n, d = A.shape
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    fmt = loss.device_matrix.plan_format()   # builds the AUTO plans before anything is timed
    x0 = np.zeros(d)
    for k in ks:
        l2s, regs = columns(k)

        def batch():
            loss.l2 = 0
            opt = Cubic_Krylov_LS_Batch(loss, k, l2=l2s, reg_coef=regs, subspace_dim=M)
            opt.run(x0, it_max)
            return opt

        def singles():
            out = []
            for c in range(k):
                loss.l2 = l2s[c]
                opt = Cubic_Krylov_LS(loss=loss, reg_coef=regs[c], label="s", subspace_dim=M, tolerance=0, tqdm=False,
                                      device_step=True)
                opt.run(x0=x0, it_max=it_max)
                out.append(opt)
            loss.l2 = 0
            return out

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            return 1e3 * (time.perf_counter() - t0), r   # both paths synchronise before they return

        for _ in range(2):   # past the placement search over the first single Lanczos calls
            bo, so = batch(), singles()
        diff = max(abs(bo.values[c] - so[c].value) / abs(so[c].value) for c in range(k))
        tb, ts = [], []
        for _ in range(alternations):
            tb.append(timed(batch)[0])
            ts.append(timed(singles)[0])
        ratios = [x / y for x, y in zip(tb, ts)]
        per = 1.0 / (it_max * k)
        row = {"shape": shape, "n": n, "d": d, "nnz": int(A.nnz), "m": M, "k": k, "it_max": it_max, "plans": fmt,
               "batch_ms_per_step_and_problem": round(statistics.median(tb) * per, 5),
               "singles_ms_per_step_and_problem": round(statistics.median(ts) * per, 5),
               "batch_ms_all": [round(x, 3) for x in tb], "singles_ms_all": [round(x, 3) for x in ts],
               "batch_over_singles": [round(r, 4) for r in ratios],
               "batch_faster_in_all": all(r < 1.0 for r in ratios),
               "batch_trials_per_step": round(float(bo.trials.sum()) / max(int(bo.its.sum()), 1), 3),
               "max_rel_value_diff_vs_singles": diff}
        print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["w8a", "rcv1", "news20"])
    ap.add_argument("--ks", nargs="+", type=int, default=[4, 8, 16])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--it-max", type=int, default=20)
    ap.add_argument("--limit", type=int, default=400, help="seconds a shape's child process may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "crn_step_block_bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("crn_step_block_bench.py needs an MI355X: it measures, it does not fall back")
        bench_shape(args.child, args.ks, args.alternations, args.it_max)
        return
    result = {"alternations": args.alternations, "it_max": args.it_max, "cases": []}
    for shape in args.shapes:   # one fresh child per shape, each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", shape,
               "--ks", *map(str, args.ks), "--alternations", str(args.alternations), "--it-max", str(args.it_max)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        rows = [json.loads(ln[4:]) for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        for row in rows:
            print(json.dumps(row), flush=True)
        result["cases"] += rows
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-4000:], file=sys.stderr)
            sys.exit(f"crn_step_block_bench.py: the {shape} step ended with status {r.returncode}; stopping")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
