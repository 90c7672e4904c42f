#!/usr/bin/env python3
"""HVP and Lanczos time of dense plans by the stored width of their values
(krcn_csr_set_value_storage), on the shapes of the reference driver's dense
datasets (run by hand on the GPU).  The protocol is tools/dense_bench.py's.

Shapes (krcn.synth.make_dense_problem): gisette 6,000 x 5,000 at 0.99 fill,
madelon 2,000 x 500 and duke 44 x 7,129 at 1.0.  Per shape three dense handles
on the same data: an fp64 handle at full width ("f64_full"), an fp64 handle
with fp32 values ("f64_v32": vectors, sums and the recurrence fp64) and an fp32
handle ("f32").  Plans are built up front, all are warmed, then the standalone
HVP is timed with device events over `--reps` back-to-back calls, alternating
the three handles `--rounds` times in this one process; the device Lanczos at
m = 10 is timed the same way over `--lz-reps` calls.  Printed per shape, one
JSON line: us per HVP of each round, medians, the algorithmic bytes
(synth.dense_hvp_bytes at the stored width; an fp64 handle's vectors stay 8
bytes) and their share of 8 TB/s, the largest relative difference of each
handle's HVP output to the CPU oracle on A32 = double(float(A)) and on A, and
whether f64_v32 beat f64_full in every round with a median gap larger than the
spread of the f64_full readings.

--parent FILE folds in a reading of the parent commit's build: a JSON-lines
file written by that commit's tools/dense_bench.py (--dtypes f64); its "dense"
readings are copied as "parent_f64_full" and the same condition is evaluated
against them.

    python tools/dense_values_bench.py [--shapes gisette madelon duke] [--parent FILE] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "krylov-cubic-regularized-newton_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

import krcn  # noqa: E402
import krcn_oracle as O  # noqa: E402
from krcn import _lib, synth  # noqa: E402

SHAPES = {"gisette": (6000, 5000, 0.99), "madelon": (2000, 500, 1.0), "duke": (44, 7129, 1.0)}
# name -> (handle dtype, values policy, bytes per stored value, bytes per vector entry)
KINDS = {"f64_full": (torch.float64, "full", 8, 8), "f64_v32": (torch.float64, "f32", 4, 8),
         "f32": (torch.float32, "full", 4, 4)}
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


def verdict(full_us, narrow_us):
    gap = statistics.median(full_us) - statistics.median(narrow_us)
    spread = max(full_us) - min(full_us)
    every = all(a < b for a, b in zip(narrow_us, full_us))
    return {"narrowed_faster_every_round": every, "median_gap_us": round(gap, 3),
            "full_spread_us": round(spread, 3), "met": every and gap > spread,
            "narrowed_over_full": round(statistics.median(narrow_us) / statistics.median(full_us), 4)}


def hvp_bytes(n, d, s_mat, s_vec):
    """synth.dense_hvp_bytes with the two images at s_mat bytes per value and the vectors at s_vec."""
    return synth.dense_hvp_bytes(n, d, s_val=s_vec) - 2 * n * d * (s_vec - s_mat)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def bench(shape, reps, lz_reps, rounds, parent):
    n, d, fill = SHAPES[shape]
    A, b = synth.make_dense_problem(n, d, fill, seed=synth.SEED)
    A32 = sp.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices, A.indptr), shape=A.shape)
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    x_h, v_h = rng.uniform(-0.01, 0.01, d), rng.standard_normal(d)
    b01_h = (b > 0).astype(np.float64)
    handles, plans, ops = {}, {}, {}
    for k, (dtype, values, _, _) in KINDS.items():
        X = krcn.DeviceCSR(A, dtype=dtype, fmt=_lib.KRCN_FORMAT_DENSE, values=values)
        X.reserve(LZ_M)   # plans (and the images) before the first compute call
        plans[k] = {"format": X.plan_format(), "info": X.plan_info(), "value_bytes": X.plan_value_bytes(),
                    "owned_mb": round(X.owned_bytes() / 1e6, 1)}
        x, v, b01 = (torch.from_numpy(a).to(dev, dtype) for a in (x_h, v_h, b01_h))
        Ax = X.matvec(x)
        handles[k] = X
        ops[k] = dict(v=v, w=X.weights(Ax), g=X.gradient(Ax, b01), y=X.empty_d(),
                      V=torch.empty((LZ_M, d), dtype=dtype, device=dev))
    hvp = {k: (lambda X=X, o=ops[k]: X.hvp(o["w"], o["v"], out=o["y"])) for k, X in handles.items()}
    lz = {k: (lambda X=X, o=ops[k]: X.lanczos(o["w"], o["g"], LZ_M, V=o["V"])) for k, X in handles.items()}
    for k in handles:   # warm: caches, the Lanczos placement search, lazily created state
        timed(hvp[k], 20)
        timed(lz[k], 8)
    diffs = {}
    for k in handles:   # each handle's y against the CPU oracle on its own w and v (widened to fp64)
        torch.cuda.synchronize()
        w, v, y = (ops[k][q].double().cpu().numpy() for q in ("w", "v", "y"))
        diffs[k] = {"vs_oracle_on_A32": rel(y, O.hvp_from_weights(A32, w, v)),
                    "vs_oracle_on_A": rel(y, O.hvp_from_weights(A, w, v))}
    t = {"hvp": {k: [] for k in KINDS}, "lanczos": {k: [] for k in KINDS}}
    for _ in range(rounds):
        for k in KINDS:
            t["hvp"][k].append(timed(hvp[k], reps))
    for _ in range(rounds):
        for k in KINDS:
            t["lanczos"][k].append(timed(lz[k], lz_reps))
    row = {"shape": shape, "n": n, "d": d, "nnz": int(A.nnz), "fill": round(A.nnz / (n * d), 4), "reps": reps,
           "lz_reps": lz_reps, "rounds": rounds, "lanczos_m": LZ_M, "plans": plans, "hvp_max_rel_diff": diffs}
    by = {k: hvp_bytes(n, d, s_mat, s_vec) for k, (_, _, s_mat, s_vec) in KINDS.items()}
    for what, scale in (("hvp", 1), ("lanczos", LZ_M)):
        row[what] = {k: summary(t[what][k], scale * by[k]) for k in KINDS}
        row[what]["condition_vs_f64_full"] = verdict(t[what]["f64_full"], t[what]["f64_v32"])
        if parent is not None:
            p_us = parent[what]["dense"]["us"]
            row[what]["parent_f64_full"] = summary(p_us, scale * by["f64_full"])
            row[what]["condition_vs_parent_f64_full"] = verdict(p_us, t[what]["f64_v32"])
            row[what]["f64_full_over_parent"] = round(statistics.median(t[what]["f64_full"]) / statistics.median(p_us), 4)
    for X in handles.values():
        X.close()
    return row


def parent_rows(path):
    rows = {}
    if path:
        with open(path) as f:
            for line in f:
                if line.strip():
                    r = json.loads(line)
                    if r["dtype"] == "f64":
                        rows[r["shape"]] = r
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--reps", type=int, default=200, help="HVPs per timed round (>= 200 for a recorded number)")
    ap.add_argument("--lz-reps", type=int, default=40, help="Lanczos calls per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="JSON lines of the parent commit's tools/dense_bench.py --dtypes f64")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dense_values_bench needs a GPU"
    parents = parent_rows(args.parent)
    for shape in args.shapes:
        line = json.dumps(bench(shape, args.reps, args.lz_reps, args.rounds, parents.get(shape)))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
