#!/usr/bin/env python3
"""Cubic_LS's CG subproblem, host-driven against krcn_cubic_cg (run by hand on the GPU).

One subproblem per shape: x = 0.5 * 1, M = 5e-4 (cubic_newton.py's first
trial: reg_coef 1e-3 times beta), r0 = 0.1, eps = 1e-8, on the synthetic w8a,
rcv1 and news20 shapes of krcn.synth.  ONE worker process per shape builds the
problem once — one loss, one handle, the gradient and the Hessian weights —
and warms both paths up:
  host    Cubic_LS.cubic_solver_root_CG as the default path has it: a Python
          root_scalar loop over krcn_cg_solve, krcn_diff_norm and krcn_dot;
  device  Cubic_LS(device_solver=True): one krcn_cubic_cg call.
The two are then timed in alternation, `--alternations` times each: a leg is a
fresh optimizer's solve between two device synchronisations, by the host's
clock.  The worker runs under its own time limit (--case-timeout seconds).

Reported per shape and path: the median leg in ms with [min, max]; Newton
iterations, CG solves and CG iterations (x-updates); the iterations the host
enqueued (host: 16 per check interval of krcn_cg_solve, from each solve's
iteration count and its loop's rule; device: ticks); vector launches per
enqueued iteration on top of the two passes (host 2, device 3) and, where the
plan tells how many launches a pass is, launches per enqueued iteration; and host
synchronisations (host: per solve one at iteration 0, one per 16 enqueued and
one at the end, one per reduction, from the same counts; device: one per batch
of ticks).  Also the ratio device / host of each alternation, whether the
device leg was the faster in all of them, and the two paths' lam and ||s||.

    python tools/cubic_cg_bench.py [--shapes w8a rcv1] [--out profiles/cubic_cg_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_EVERY = 16     # kCgCheckEvery, csrc/krcn_cg.hip


def worker(args):
    sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
    import numpy as np
    import torch

    from krcn import synth
    from optimizer.cubic import Cubic_LS
    from optimizer.loss import LogisticRegression

    A, b = synth.make_problem(args.worker)
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    X = loss.device_matrix
    x = loss.to_device(np.full(A.shape[1], 0.5))
    grad = loss.gradient(x)
    batch = int(os.environ.get("KRCN_CGN_BATCH", "16"))

    # launches of a pass: its main launch, and the slice combine of a sliced plan (csrc/krcn_pass.hpp,
    # combine_arrays; a sliced jagged plan combines only over several slice groups, which plan_info does not tell)
    fmts, plans = X.plan_format(), X.plan_info()

    def pass_launches(name):
        fmt, slices = fmts[name], abs(plans[name][0])
        if fmt == "window-accum":
            return 1
        if fmt == "window-slices":
            return 2
        if fmt == "jagged" and slices > 1:
            return None
        return 2 if slices > 1 else 1

    passes = [pass_launches("pass1"), pass_launches("pass2")]
    pass_total = None if None in passes else sum(passes)

    counts = {}
    cg_solve, dot, diff_norm, cubic_cg = X.cg_solve, X.dot, X.diff_norm, X.cubic_cg

    def counted_cg_solve(*a, **k):
        out, info = cg_solve(*a, **k)
        counts["solves"] += 1
        counts["cg_iterations"] += info.iterations
        enq = CHECK_EVERY * -(-info.iterations // CHECK_EVERY)
        counts["enqueued"] += enq
        counts["syncs"] += enq // CHECK_EVERY + 2
        return out, info

    def counted_reduction(fn):
        def f(*a, **k):
            counts["syncs"] += 1
            return fn(*a, **k)
        return f

    def counted_cubic_cg(*a, **k):
        out, info = cubic_cg(*a, **k)
        counts["solves"] += info.cg_solves
        counts["cg_iterations"] += info.cg_iterations
        counts["enqueued"] += info.ticks
        counts["syncs"] += -(-info.ticks // batch)
        counts["status"] = info.solver_status
        return out, info

    X.cg_solve, X.dot, X.diff_norm = counted_cg_solve, counted_reduction(dot), counted_reduction(diff_norm)
    X.cubic_cg = counted_cubic_cg

    def leg(device_solver):
        counts.update(solves=0, cg_iterations=0, enqueued=0, syncs=0, status=0)
        opt = Cubic_LS(loss=loss, reg_coef=1e-3, label="CRN", cubic_solver="CG", tolerance=1e-8, tqdm=False,
                       device_solver=device_solver)
        opt.x, opt.grad = x, grad
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s, its, lam, dec = opt.cubic_solver_root_CG(opt.reg_coef * opt.beta, opt.solver_it_max, opt.solver_eps,
                                                    r0=opt.r0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dict(counts, ms=1e3 * dt, newton_iterations=int(its), lam=float(lam), model_decrease=float(dec),
                    s_norm=float(diff_norm(s)), cg_unconverged=int(opt.cg_unconverged))

    def summary(legs, device_solver):
        ms = [l["ms"] for l in legs]
        last = legs[-1]
        return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "newton_iterations": last["newton_iterations"], "cg_solves": last["solves"],
                "cg_iterations": last["cg_iterations"], "enqueued_iterations": last["enqueued"],
                "vector_launches_per_iteration": 3 if device_solver else 2,
                "launches_per_iteration": None if pass_total is None else pass_total + (3 if device_solver else 2),
                "synchronisations": last["syncs"],
                "cg_unconverged": last["cg_unconverged"], "solver_status": last["status"], "lam": last["lam"],
                "model_decrease": last["model_decrease"], "s_norm": last["s_norm"]}

    for _ in range(args.warm_legs):
        leg(False)
        leg(True)
    legs = {False: [], True: []}
    for _ in range(args.alternations):
        for device_solver in (False, True):
            legs[device_solver].append(leg(device_solver))
    ratios = [d["ms"] / h["ms"] for h, d in zip(legs[False], legs[True])]
    print(json.dumps({"shape": args.worker, "n": A.shape[0], "d": A.shape[1], "nnz": int(A.nnz), "M": 5e-4,
                      "alternations": args.alternations, "tick_batch": batch, "plan_format": fmts,
                      "plan_info": plans,
                      "host": summary(legs[False], False), "device": summary(legs[True], True),
                      "device_over_host": [round(r, 4) for r in ratios],
                      "device_faster_in_all": all(r < 1.0 for r in ratios)}), flush=True)


def bench_shape(shape, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--warm-legs", str(args.warm_legs),
           "--alternations", str(args.alternations)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.case_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"the {shape} worker ended with exit status {p.returncode}")
    return [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["w8a", "rcv1", "news20"])
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--warm-legs", type=int, default=2)
    ap.add_argument("--case-timeout", type=float, default=240.0, help="seconds one shape's worker may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    result = {"cases": []}
    for shape in args.shapes:      # (a worker that fails or runs out of time ends the run: nothing is retried)
        for r in bench_shape(shape, args):
            print(json.dumps(r), flush=True)
            result["cases"].append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
