#!/usr/bin/env python3
"""Krylov-CRN step time, host step against device step (run by hand on the GPU).

For every case (synthetic shape : subspace_dim; default w8a:10 rcv1:10 rcv1:50
news20:100) two worker processes each build the problem and warm up, one with
the host step (Cubic_Krylov_LS as the parent commit has it: host subproblem,
host line search) and one with Cubic_Krylov_LS(device_step=True).  The two are
then timed in alternation, `--alternations` times each: a leg is a fresh
optimizer's run(x0, it_max=--steps) between two device synchronisations, by the
host's clock, so a step holds everything run() does for it (the stopping
test's clone and norm_diff included: tolerance = 1e-9 as the tests run it).
Reported per case and path: the median leg in ms per step with min and max,
the mean backtracking trials per step (from reg_coef's ratio step to step),
the final value, and per alternation whether the device leg was the faster.

--repo DIR takes the host leg's packages (krcn, optimizer) from another
checkout, the parent commit's, built there; the host leg uses nothing that
commit lacks.  Without it both legs come from this checkout.

Also reported: the subproblem kernel alone (DeviceCSR.cubic_tridiag on a
diagonally dominant tridiagonal T) at m = 1, 10, 100 and 500 by device events
around the call; the m = 1 row is the call's own cost (two staging copies, two
launches, one synchronisation), which the other rows contain.

    python tools/crn_step_bench.py [--cases w8a:10 rcv1:10] [--repo DIR] [--out FILE]
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
    """One path of one case: answers every line on stdin with one JSON line."""
    sys.path.insert(0, os.path.join(args.repo or REPO, "krylov-cubic-regularized-newton_amd"))
    import numpy as np
    import torch

    from krcn import synth
    from optimizer.cubic import Cubic_Krylov_LS
    from optimizer.loss import LogisticRegression

    shape, m = args.worker_case.split(":")
    m = int(m)
    A, b = synth.make_problem(shape)
    loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True)
    x0 = np.full(A.shape[1], 0.5)
    extra = {"device_step": True} if args.worker == "device" else {}

    def leg(steps):
        loss.reset()
        opt = Cubic_Krylov_LS(loss=loss, reg_coef=1e-3, label="k", subspace_dim=m, tolerance=1e-9, tqdm=False,
                              **extra)
        regs = [opt.reg_coef]
        step = opt.step

        def recording_step():
            step()
            regs.append(opt.reg_coef)

        opt.step = recording_step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.run(x0=x0, it_max=steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        trials = [round(float(np.log2(regs[k + 1] / (regs[k] * opt.beta)))) for k in range(len(regs) - 1)]
        return {"ms_per_step": 1e3 * dt / max(opt.it, 1), "steps": int(opt.it),
                "mean_trials": float(np.mean(trials)) if trials else 0.0, "value": float(opt.value)}

    for _ in range(args.warm_legs):
        leg(args.steps)
    print(json.dumps({"ready": True, "n": A.shape[0], "d": A.shape[1], "nnz": int(A.nnz)}), flush=True)
    for line in sys.stdin:
        if line.strip() == "go":
            print(json.dumps(leg(args.steps)), flush=True)
        else:
            break


def start_worker(path, case, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", path, "--worker-case", case, "--steps",
           str(args.steps), "--warm-legs", str(args.warm_legs)]
    if path == "host" and args.repo:
        cmd += ["--repo", os.path.abspath(args.repo)]
    p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    return p


def ask(p, msg=None):
    if msg is not None:
        p.stdin.write(msg + "\n")
        p.stdin.flush()
    line = p.stdout.readline()
    if not line:
        raise RuntimeError(f"a worker ended early (exit status {p.poll()})")
    return json.loads(line)


def summary(legs):
    ms = [l["ms_per_step"] for l in legs]
    return {"ms_per_step": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "steps": legs[-1]["steps"], "mean_trials": round(legs[-1]["mean_trials"], 3), "value": legs[-1]["value"]}


def bench_case(case, args):
    workers = {path: start_worker(path, case, args) for path in ("host", "device")}
    try:
        dims = {path: ask(p) for path, p in workers.items()}["host"]
        legs = {"host": [], "device": []}
        for _ in range(args.alternations):
            for path in ("host", "device"):
                legs[path].append(ask(workers[path], "go"))
    finally:
        for p in workers.values():
            try:
                p.stdin.close()
            except OSError:
                pass
            p.wait(timeout=60)
    shape, m = case.split(":")
    ratios = [d["ms_per_step"] / h["ms_per_step"] for h, d in zip(legs["host"], legs["device"])]
    return {"shape": shape, "subspace_dim": int(m), "n": dims["n"], "d": dims["d"], "nnz": dims["nnz"],
            "steps": args.steps, "alternations": args.alternations, "host_from": args.repo or "this checkout",
            "host": summary(legs["host"]), "device": summary(legs["device"]),
            "device_over_host": [round(r, 4) for r in ratios],
            "device_faster_in_all": all(r < 1.0 for r in ratios)}


# ------------------------------------------------------- the kernel alone
def bench_kernel(ms_list=(1, 10, 100, 500), reps=20):
    sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
    import numpy as np
    import scipy.sparse as sp
    import torch

    import krcn
    X = krcn.DeviceCSR(sp.identity(8, format="csr"))
    out = []
    for m in ms_list:
        rng = np.random.default_rng(m)
        al = 0.1 + rng.uniform(0.0, 0.2, m)
        be = rng.uniform(0.01, 0.04, max(m - 1, 0))
        X.cubic_tridiag(al, be, 0.05, 1e-3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            s, info = X.cubic_tridiag(al, be, 0.05, 1e-3)
        e1.record()
        torch.cuda.synchronize()
        out.append({"m": m, "us_per_call": round(1e3 * e0.elapsed_time(e1) / reps, 2),
                    "newton_iterations": int(info.solver_it), "solver_status": int(info.solver_status)})
    X.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["w8a:10", "rcv1:10", "rcv1:50", "news20:100"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--warm-legs", type=int, default=1)
    ap.add_argument("--repo", default=None, help="checkout (built) whose krcn / optimizer packages run the host leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--worker", choices=["host", "device"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker-case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    result = {"cases": [], "subproblem_kernel": []}
    for case in args.cases:
        r = bench_case(case, args)
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
