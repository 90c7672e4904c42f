#!/usr/bin/env python3
"""HVP and Lanczos time of the dense plan format against the AUTO plan, on the
shapes of the reference driver's dense datasets (run by hand on the GPU).

Shapes (krcn.synth.make_dense_problem): gisette 6,000 x 5,000 at 0.99 fill,
madelon 2,000 x 500 and duke 44 x 7,129 at 1.0, each in fp64 and fp32.  Per
(shape, dtype) one AUTO handle and one dense handle are built on the same data
with their plans built up front, both are warmed, and then the standalone HVP
is timed with device events over `--reps` back-to-back calls, alternating
AUTO / dense `--rounds` times in this one process; the device Lanczos at
m = 10 (the reference driver's memory_size) is timed the same way over
`--lz-reps` calls.  Printed per (shape, dtype), one JSON line: us per HVP and
HVP/s of each round, the medians, the algorithmic bytes (dense
2 n d s + s (2d + 3n); CSR synth.hvp_bytes) and their share of 8 TB/s, the
largest relative difference of the two handles' HVP outputs on the timed
inputs, and whether dense beat AUTO in every round with a median gap larger
than the spread of the AUTO readings.

    python tools/dense_bench.py [--shapes gisette madelon duke] [--dtypes f64 f32] [--out FILE]

KRCN_LIB=PATH runs another build of the library (the A/B variants of DESIGN.md §11).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import krcn  # noqa: E402
from krcn import _lib, synth  # noqa: E402

SHAPES = {"gisette": (6000, 5000, 0.99), "madelon": (2000, 500, 1.0), "duke": (44, 7129, 1.0)}
DTYPES = {"f64": (torch.float64, 8), "f32": (torch.float32, 4)}
HBM_BYTES_PER_S = 8e12
LZ_M = 10


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps   # us per call


def summary(us, nbytes):
    med = statistics.median(us)
    return {"us": [round(v, 3) for v in us], "us_median": round(med, 3), "per_s": round(1e6 / med, 1),
            "bytes": int(nbytes), "share_of_8TBps": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 4)}


def verdict(auto_us, dense_us):
    gap = statistics.median(auto_us) - statistics.median(dense_us)
    spread = max(auto_us) - min(auto_us)
    return {"dense_faster_every_round": all(d < a for a, d in zip(auto_us, dense_us)),
            "median_gap_us": round(gap, 3), "auto_spread_us": round(spread, 3),
            "met": all(d < a for a, d in zip(auto_us, dense_us)) and gap > spread,
            "dense_over_auto": round(statistics.median(dense_us) / statistics.median(auto_us), 4)}


def bench(shape, dname, reps, lz_reps, rounds):
    n, d, fill = SHAPES[shape]
    dtype, vs = DTYPES[dname]
    A, b = synth.make_dense_problem(n, d, fill, seed=synth.SEED)
    dev = torch.device("cuda", torch.cuda.current_device())
    handles = {"auto": krcn.DeviceCSR(A, dtype=dtype), "dense": krcn.DeviceCSR(A, dtype=dtype, fmt=_lib.KRCN_FORMAT_DENSE)}
    plans = {}
    for k, X in handles.items():   # plans (and the dense images) before the first compute call
        X.reserve(LZ_M)
        plans[k] = {"format": X.plan_format(), "info": X.plan_info(), "owned_mb": round(X.owned_bytes() / 1e6, 1)}
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(-0.01, 0.01, d)).to(dev, dtype)
    v = torch.from_numpy(rng.standard_normal(d)).to(dev, dtype)
    b01 = torch.from_numpy((b > 0).astype(np.float64)).to(dev, dtype)
    ops = {}
    for k, X in handles.items():
        Ax = X.matvec(x)
        ops[k] = dict(w=X.weights(Ax), g=X.gradient(Ax, b01), y=X.empty_d(),
                      V=torch.empty((LZ_M, d), dtype=dtype, device=dev))
    hvp = {k: (lambda X=X, o=ops[k]: X.hvp(o["w"], v, out=o["y"])) for k, X in handles.items()}
    lz = {k: (lambda X=X, o=ops[k]: X.lanczos(o["w"], o["g"], LZ_M, V=o["V"])) for k, X in handles.items()}
    for k in handles:   # warm: caches, the Lanczos placement search, lazily created state
        timed(hvp[k], 20)
        timed(lz[k], 8)
    ya, yd = ops["auto"]["y"].double(), ops["dense"]["y"].double()
    diff = float((ya - yd).abs().max() / ya.abs().max())
    t = {"hvp": {"auto": [], "dense": []}, "lanczos": {"auto": [], "dense": []}}
    for _ in range(rounds):
        for k in ("auto", "dense"):
            t["hvp"][k].append(timed(hvp[k], reps))
    for _ in range(rounds):
        for k in ("auto", "dense"):
            t["lanczos"][k].append(timed(lz[k], lz_reps))
    by = {"auto": synth.hvp_bytes(n, d, int(A.nnz), s_val=vs), "dense": synth.dense_hvp_bytes(n, d, s_val=vs)}
    row = {"shape": shape, "dtype": dname, "n": n, "d": d, "nnz": int(A.nnz), "fill": round(A.nnz / (n * d), 4),
           "reps": reps, "lz_reps": lz_reps, "rounds": rounds, "lanczos_m": LZ_M, "plans": plans,
           "hvp_max_rel_diff": diff}
    for what, scale in (("hvp", 1), ("lanczos", LZ_M)):
        row[what] = {k: summary(t[what][k], scale * by[k]) for k in ("auto", "dense")}
        row[what]["condition"] = verdict(t[what]["auto"], t[what]["dense"])
    for X in handles.values():
        X.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--reps", type=int, default=200, help="HVPs per timed round (>= 200 for a recorded number)")
    ap.add_argument("--lz-reps", type=int, default=40, help="Lanczos calls per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dense_bench needs a GPU"
    for shape in args.shapes:
        for dname in args.dtypes:
            line = json.dumps(bench(shape, dname, args.reps, args.lz_reps, args.rounds))
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
