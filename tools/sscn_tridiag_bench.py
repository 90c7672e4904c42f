#!/usr/bin/env python3
"""SSCN's device step over one tridiagonal reduction: its pieces, its solver
against the Cholesky solver, and its step against the step it replaces (run by
hand on the GPU).  The method is tools/sscn_step_bench.py's.

Steps.  For every case (synthetic shape : subspace_dim : baseline; default
w8a:100:cholesky rcv1:500:host rcv1:1000:host news20:500:host news20:1000:host)
ONE resident worker process per shape builds the problem once — one loss, one
handle — and warms both paths up: the baseline (`host`: SSCN as the default
path has it, coordinate kernels, host cubic_solver_root — its spsolve branch
from 500 columns on —, host line search; `cholesky`: SSCN(device_step=True))
and SSCN(device_step=True, subproblem="tridiag").  The two are timed in
alternation, `--alternations` times each, with the same seed: a leg is a fresh
optimizer's run(x0, it_max=steps) on that handle between two device
synchronisations, by the host's clock.  Reported per case and path: the median
leg in ms per step with every value, the mean backtracking trials per step, the
final value, the ratio tridiag / baseline of each alternation, whether the
tridiag leg was the faster in all of them, and whether the final values agree
to 1e-10.

Pieces, by device events over `--reps` calls on pinned host arrays, per call in
microseconds, medians of `--alternations` rounds with every value:
  reduction        DeviceCSR.dense_tridiag (staging of H and g, fill, the column
                   launches, the closing kernel, alphas and betas back)
  tridiag solve    DeviceCSR.cubic_tridiag on the reduction's alphas and betas
  reduce + solve   DeviceCSR.cubic_dense_tridiag (reduction, solve, back-transform)
  back-transform   reduce + solve minus the two above (a difference of calls:
                   each carries its own staging copies and synchronisation)
and DeviceCSR.cubic_dense against DeviceCSR.cubic_dense_tridiag at k = 10, 32,
64, 100, 128 on the same blocks.

    python tools/sscn_tridiag_bench.py [--cases w8a:100:cholesky] [--out profiles/sscn_tridiag_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ worker
def worker(args):
    """One shape: every (subspace_dim, baseline) of it on one handle; one JSON line per case."""
    sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
    import numpy as np
    import torch

    from krcn import synth
    from optimizer.cubic import SSCN
    from optimizer.loss import LogisticRegression

    A, b = synth.make_problem(args.worker)
    loss = LogisticRegression(A.tocsc(), b, l1=0, l2=0, store_mat_vec_prod=True)
    x0 = np.full(A.shape[1], 0.5)

    def leg(k, path, steps):
        loss.reset()
        kw = {"host": {}, "cholesky": {"device_step": True},
              "tridiag": {"device_step": True, "subproblem": "tridiag"}}[path]
        opt = SSCN(loss=loss, reg_coef=1e-3, label="SSCN", subspace_dim=k, tolerance=1e-9, tqdm=False, **kw)
        trials, step = [], opt.step

        def recording_step():
            step()
            trials.append(opt.last_trials)

        opt.step = recording_step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.run(x0=x0, it_max=steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"ms_per_step": 1e3 * dt / max(opt.it, 1), "steps": int(opt.it),
                "mean_trials": float(np.mean(trials)) if trials else 0.0, "value": float(opt.value)}

    def summary(legs):
        ms = [l["ms_per_step"] for l in legs]
        return {"ms_per_step": round(statistics.median(ms), 4), "ms_all": [round(m, 4) for m in ms],
                "steps": legs[-1]["steps"], "mean_trials": round(legs[-1]["mean_trials"], 3),
                "value": legs[-1]["value"]}

    for spec in args.dims:
        k, base = spec.split(":")
        k = int(k)
        steps = args.steps if k < 500 else args.steps_large
        for _ in range(args.warm_legs):
            leg(k, base, steps)
            leg(k, "tridiag", steps)
        legs = {base: [], "tridiag": []}
        for _ in range(args.alternations):
            for path in (base, "tridiag"):
                legs[path].append(leg(k, path, steps))
        ratios = [t["ms_per_step"] / h["ms_per_step"] for h, t in zip(legs[base], legs["tridiag"])]
        vb, vt = legs[base][-1]["value"], legs["tridiag"][-1]["value"]
        print(json.dumps({"shape": args.worker, "subspace_dim": k, "baseline": base, "n": A.shape[0],
                          "d": A.shape[1], "nnz": int(A.nnz), "steps": steps, "alternations": args.alternations,
                          base: summary(legs[base]), "tridiag": summary(legs["tridiag"]),
                          "tridiag_over_baseline": [round(r, 4) for r in ratios],
                          "tridiag_faster_in_all": all(r < 1.0 for r in ratios),
                          "values_agree_1e-10": abs(vb - vt) <= 1e-10 * abs(vb)}), flush=True)


def bench_shape(shape, dims, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--dims", *dims,
           "--steps", str(args.steps), "--steps-large", str(args.steps_large), "--warm-legs", str(args.warm_legs),
           "--alternations", str(args.alternations)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.case_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"the {shape} worker ended with exit status {p.returncode}")
    return [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]


# ------------------------------------------------------------- the pieces
def bench_pieces(args, ks=(10, 32, 64, 100, 128, 257, 512, 1024)):
    sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
    import numpy as np
    import scipy.sparse as sp
    import torch

    import krcn
    X = krcn.DeviceCSR(sp.identity(8, format="csr"))

    def pinned(a):
        t = torch.empty(a.shape, dtype=torch.float64, pin_memory=True)
        out = t.numpy()
        out[...] = a
        return t, out

    def per_call(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.reps, r

    out = []
    for k in ks:
        rng = np.random.default_rng(k)
        B = rng.uniform(-0.02, 0.02, (k, k))
        keepH, H = pinned((B + B.T) / 2 + np.diag(0.1 + rng.uniform(0.0, 0.2, k) + 0.02 * k))
        keepg, g = pinned(0.05 * rng.standard_normal(k))
        al, be, _ = X.dense_tridiag(H, g)
        rounds = {"reduction": [], "tridiag_solve": [], "reduce_solve": [], "cholesky": []}
        info = infoc = None
        for _ in range(args.alternations):
            rounds["reduction"].append(per_call(lambda: X.dense_tridiag(H, g))[0])
            rounds["tridiag_solve"].append(per_call(lambda: X.cubic_tridiag(al, be[1:], float(be[0]), 1e-3))[0])
            t, (_, info) = per_call(lambda: X.cubic_dense_tridiag(H, g, 1e-3))
            rounds["reduce_solve"].append(t)
            if k <= 128:
                t, (_, infoc) = per_call(lambda: X.cubic_dense(H, g, 1e-3))
                rounds["cholesky"].append(t)
        med = {n: statistics.median(v) for n, v in rounds.items() if v}
        r = {"k": k, "reps": args.reps, "newton_iterations": int(info.solver_it),
             "solver_status": int(info.solver_status),
             "us_per_call": {n: round(m, 2) for n, m in med.items()},
             "us_all": {n: [round(x, 2) for x in v] for n, v in rounds.items() if v},
             "us_back_transform_by_difference": round(med["reduce_solve"] - med["reduction"] - med["tridiag_solve"], 2)}
        if infoc is not None:
            r["cholesky_newton_iterations"] = int(infoc.solver_it)
            r["tridiag_over_cholesky"] = round(med["reduce_solve"] / med["cholesky"], 4)
        out.append(r)
        del keepH, keepg
    X.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="*", default=["w8a:100:cholesky", "rcv1:500:host", "rcv1:1000:host",
                                                   "news20:500:host", "news20:1000:host"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--steps-large", type=int, default=3, help="steps of a leg at 500 columns and more")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--warm-legs", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--case-timeout", type=float, default=400.0, help="seconds one shape's worker may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pieces", action="store_true")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dims", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    shapes = {}
    for case in args.cases:
        shape, k, base = case.split(":")
        if base not in ("host", "cholesky"):
            ap.error(f"baseline of {case} must be host or cholesky")
        shapes.setdefault(shape, []).append(f"{k}:{base}")
    result = {"cases": [], "pieces": []}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    if not args.no_pieces:
        result["pieces"] = bench_pieces(args)
        for r in result["pieces"]:
            print(json.dumps(r), flush=True)
        save()
    for shape, dims in shapes.items():
        for r in bench_shape(shape, dims, args):
            print(json.dumps(r), flush=True)
            result["cases"].append(r)
        save()


if __name__ == "__main__":
    main()
