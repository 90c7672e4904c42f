#!/usr/bin/env python3
"""SSCN step time, host step against device step (run by hand on the GPU).

For every case (synthetic shape : subspace_dim; default w8a:10 w8a:100
news20:10 news20:100) ONE resident worker process per shape builds the problem
once — one loss, one handle — and warms both paths up: SSCN as the default
path has it (coordinate kernels, host cubic_solver_root, host line search) and
SSCN(device_step=True).  The two are then timed in alternation,
`--alternations` times each, with the same seed: a leg is a fresh optimizer's
run(x0, it_max=--steps) on that handle between two device synchronisations, by
the host's clock, so a step holds everything run() does for it.  The worker
runs under its own time limit (--case-timeout seconds per shape).
Reported per case and path: the median leg in ms per step with [min, max], the
mean backtracking trials per step (from reg_coef's ratio step to step), the
final value, the ratio device / host of each alternation, and whether the
device leg was the faster in all of them.

Also reported: the subproblem kernel alone (DeviceCSR.cubic_dense on a
diagonally dominant dense block) at k = 1, 10, 32, 64, 100 and 128 by device
events over 20 calls: per call, and per Newton iteration after the k = 1 call's
cost (staging copies, two launches, one synchronisation) is taken off.

    python tools/sscn_step_bench.py [--cases w8a:10 news20:10] [--out profiles/sscn_step_bench.json]
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
    """One shape: every subspace_dim of it, both paths on one handle; one JSON line per case."""
    sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
    import numpy as np
    import torch

    from krcn import synth
    from optimizer.cubic import SSCN
    from optimizer.loss import LogisticRegression

    A, b = synth.make_problem(args.worker)
    loss = LogisticRegression(A.tocsc(), b, l1=0, l2=0, store_mat_vec_prod=True)
    x0 = np.full(A.shape[1], 0.5)

    def leg(k, device_step):
        loss.reset()
        opt = SSCN(loss=loss, reg_coef=1e-3, label="SSCN", subspace_dim=k, tolerance=1e-9, tqdm=False,
                   device_step=device_step)
        regs = [opt.reg_coef]
        step = opt.step

        def recording_step():
            step()
            regs.append(opt.reg_coef)

        opt.step = recording_step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.run(x0=x0, it_max=args.steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        trials = [round(float(np.log2(regs[i + 1] / max(regs[i] * opt.beta, np.finfo(float).eps))))
                  for i in range(len(regs) - 1)]
        return {"ms_per_step": 1e3 * dt / max(opt.it, 1), "steps": int(opt.it),
                "mean_trials": float(np.mean(trials)) if trials else 0.0, "value": float(opt.value)}

    def summary(legs):
        ms = [l["ms_per_step"] for l in legs]
        return {"ms_per_step": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                "ms_max": round(max(ms), 4), "steps": legs[-1]["steps"],
                "mean_trials": round(legs[-1]["mean_trials"], 3), "value": legs[-1]["value"]}

    for k in args.dims:
        for _ in range(args.warm_legs):
            leg(k, False)
            leg(k, True)
        legs = {False: [], True: []}
        for _ in range(args.alternations):
            for device_step in (False, True):
                legs[device_step].append(leg(k, device_step))
        ratios = [d["ms_per_step"] / h["ms_per_step"] for h, d in zip(legs[False], legs[True])]
        print(json.dumps({"shape": args.worker, "subspace_dim": k, "n": A.shape[0], "d": A.shape[1],
                          "nnz": int(A.nnz), "steps": args.steps, "alternations": args.alternations,
                          "host": summary(legs[False]), "device": summary(legs[True]),
                          "device_over_host": [round(r, 4) for r in ratios],
                          "device_faster_in_all": all(r < 1.0 for r in ratios)}), flush=True)


def bench_shape(shape, dims, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--dims", *[str(k) for k in dims],
           "--steps", str(args.steps), "--warm-legs", str(args.warm_legs), "--alternations", str(args.alternations)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.case_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"the {shape} worker ended with exit status {p.returncode}")
    return [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]


# ------------------------------------------------------- the kernel alone
def bench_kernel(ks=(1, 10, 32, 64, 100, 128), reps=20):
    sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
    import numpy as np
    import scipy.sparse as sp
    import torch

    import krcn
    X = krcn.DeviceCSR(sp.identity(8, format="csr"))
    out = []
    for k in ks:
        rng = np.random.default_rng(k)
        B = rng.uniform(-0.02, 0.02, (k, k))
        H = (B + B.T) / 2 + np.diag(0.1 + rng.uniform(0.0, 0.2, k) + 0.02 * k)
        g = 0.05 * rng.standard_normal(k)
        X.cubic_dense(H, g, 1e-3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            s, info = X.cubic_dense(H, g, 1e-3)
        e1.record()
        torch.cuda.synchronize()
        out.append({"k": k, "us_per_call": round(1e3 * e0.elapsed_time(e1) / reps, 2),
                    "newton_iterations": int(info.solver_it), "solver_status": int(info.solver_status)})
    X.close()
    base = out[0]
    for r in out:   # (a solve factors once per Newton iteration and once more for the closing solve)
        fact = r["newton_iterations"] + 1
        r["us_per_newton_iteration"] = round(max(r["us_per_call"] - base["us_per_call"], 0.0) / fact, 2) \
            if r is not base else None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["w8a:10", "w8a:100", "news20:10", "news20:100"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--warm-legs", type=int, default=1)
    ap.add_argument("--case-timeout", type=float, default=240.0, help="seconds one shape's worker may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dims", nargs="+", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    shapes = {}
    for case in args.cases:
        shape, k = case.split(":")
        shapes.setdefault(shape, []).append(int(k))
    result = {"cases": [], "subproblem_kernel": []}
    for shape, dims in shapes.items():
        for r in bench_shape(shape, dims, args):
            print(json.dumps(r), flush=True)
            result["cases"].append(r)
    if not args.no_kernel:
        result["subproblem_kernel"] = bench_kernel()
        print(json.dumps({"subproblem_kernel": result["subproblem_kernel"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
