#!/usr/bin/env python3
"""The dense Hessian as one Gram product against the builds it replaces (run by
hand on the GPU).

Shapes (krcn.synth.make_dense_problem, format="dense", w at x = 0.5 * 1):
gisette 6,000 x 5,000 at 0.99 fill in fp64 and in fp64 with values="f32",
madelon 2,000 x 500 and duke 44 x 7,129 at 1.0 in fp64.  One resident warm
process per run; every leg is timed by device events, `--alternations` times in
alternation with the other leg of its shape:

  gram       DeviceCSR.hessian_gram(w, l2) into a resident (d, d) tensor
  block16    gisette and duke: the device part of LogisticRegression.hessian(x,
             block=16): d / 16 krcn_hvp_block calls over unit vectors into a
             resident (d, d) tensor (the parent commit's code)
  coord      madelon (d <= KRCN_COORD_MAX): DeviceCSR.coord_hessian(range(d)),
             which ends with its copy of H to the host

Reported per shape: us per call of each leg (median and every alternation), the
split the rule chose, n d (d + 1) flop over the Gram call's time, whether the
Gram call was the faster in every alternation, and the largest difference of the
entries between the legs relative to the largest entry.

--sweep N D: the forced split 1, 2, 3, 4, 6, 8, 12, 16 and the rule's own on one
N x D problem with few tiles (the resident-CU question).

    python tools/hessian_bench.py [--shapes gisette madelon duke] [--sweep 50000 1100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))

SHAPES = {"gisette": (6000, 5000, 0.99), "madelon": (2000, 500, 1.0), "duke": (44, 7129, 1.0)}
L2 = 0.01


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def setup(A, values):
    import torch

    import krcn
    X = krcn.DeviceCSR(A, fmt=5, values=values)
    X.plan_info()   # the images are built here
    x = torch.full((X.d,), 0.5, dtype=torch.float64, device=X.device)
    Ax = X.matvec(x)
    return X, Ax, X.weights(Ax)


def block16_build(X, w, H, E):
    import torch
    d, k = X.d, E.shape[1]
    for c0 in range(0, d, k):
        kc = min(k, d - c0)
        Ec = E if kc == k else torch.zeros((d, kc), dtype=torch.float64, device=X.device)
        diag = torch.arange(kc, device=X.device)
        Ec[c0 + diag, diag] = 1.0
        H[:, c0:c0 + kc] = X.hvp_block(w, Ec, l2=L2)
        Ec[c0 + diag, diag] = 0.0


def bench_shape(name, A, values, alternations, gram_reps):
    import numpy as np
    import torch

    import krcn
    from krcn import _lib
    n, d = A.shape
    X, Ax, w = setup(A, values)
    Hg = torch.empty((d, d), dtype=torch.float64, device=X.device)
    geo = krcn.gram_geometry(d, n)

    def gram():
        X.hessian_gram(w, l2=L2, out=Hg)

    if d <= _lib.KRCN_COORD_MAX:
        other_name, cols, box = "coord", np.arange(d), {}

        def other():
            box["H"] = X.coord_hessian(cols, Ax, L2)
    else:
        other_name = "block16"
        Hb = torch.empty((d, d), dtype=torch.float64, device=X.device)
        E = torch.zeros((d, 16), dtype=torch.float64, device=X.device)

        def other():
            block16_build(X, w, Hb, E)

    gram()
    other()
    torch.cuda.synchronize()
    ref = torch.from_numpy(box["H"]).to(X.device) if other_name == "coord" else Hb
    diff = float((Hg - ref).abs().max() / ref.abs().max())
    tg, to = [], []
    for _ in range(alternations):
        tg.append(timed(gram, gram_reps))
        to.append(timed(other, 1))
    us = statistics.median(tg)
    row = {"shape": name, "n": n, "d": d, "values": values, "stored_bytes": X.plan_value_bytes()["pass2"],
           "split": geo["split"], "tiles": geo["tiles"], "slabs": geo["slabs"],
           "gram_us": round(us, 1), "gram_us_all": [round(v, 1) for v in tg],
           "gram_tflops": round(n * d * (d + 1) / (us * 1e-6) / 1e12, 3),
           "other": other_name, "other_us": round(statistics.median(to), 1), "other_us_all": [round(v, 1) for v in to],
           "gram_over_other": [round(g / o, 5) for g, o in zip(tg, to)],
           "gram_faster_in_all": all(g < o for g, o in zip(tg, to)),
           "max_diff_rel_to_largest_entry": diff}
    print(json.dumps(row), flush=True)
    X.close()
    return row


def sweep(n, d, alternations, gram_reps):
    import torch

    import krcn
    from krcn import synth
    A, _ = synth.make_dense_problem(n, d, 1.0)
    X, _, w = setup(A, "full")
    H = torch.empty((d, d), dtype=torch.float64, device=X.device)
    auto = krcn.gram_geometry(d, n)
    splits = sorted({1, 2, 3, 4, 6, 8, 12, 16, auto["split"]})

    def run():
        X.hessian_gram(w, l2=L2, out=H)

    times = {s: [] for s in splits}
    for s in splits:                      # warm every split (and grow the workspace to the largest)
        X.set_gram_split(s)
        run()
    for _ in range(alternations):
        for s in splits:
            X.set_gram_split(s)
            times[s].append(timed(run, gram_reps))
    rows = [{"split": s, "workgroups": auto["tiles"] * s, "us": round(statistics.median(times[s]), 1),
             "us_all": [round(v, 1) for v in times[s]],
             "tflops": round(n * d * (d + 1) / (statistics.median(times[s]) * 1e-6) / 1e12, 3)} for s in splits]
    out = {"n": n, "d": d, "tiles": auto["tiles"], "slabs": auto["slabs"], "auto_split": auto["split"], "splits": rows}
    print(json.dumps(out), flush=True)
    X.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="*", default=["gisette", "madelon", "duke"])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--gram-reps", type=int, default=3)
    ap.add_argument("--sweep", nargs=2, type=int, default=None, metavar=("N", "D"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("hessian_bench.py needs an MI355X: it measures, it does not fall back")
    from krcn import synth
    result = {"alternations": args.alternations, "gram_reps": args.gram_reps, "l2": L2, "cases": []}
    for name in args.shapes:
        n, d, fill = SHAPES[name]
        A, _ = synth.make_dense_problem(n, d, fill)
        for values in (("full", "f32") if name == "gisette" else ("full",)):
            result["cases"].append(bench_shape(name, A, values, args.alternations, args.gram_reps))
    if args.sweep:
        result["sweep"] = sweep(*args.sweep, args.alternations, args.gram_reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
