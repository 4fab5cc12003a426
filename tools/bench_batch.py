#!/usr/bin/env python3
"""Batched small-n solve against a loop of single solves: aggregate iterations per second of one
Batch.minimize over B problems and of Context.minimize called once per problem, the same problems
(Rosenbrock, n = 1e4, m = 5, backtracking, x0 = x0_uniform(n, seed p + 1, -2, 2)), a fixed iteration
count (tolerance 0), for B in {1, 16, 256, 1024}. The two alternate in one process after a warm-up
of both; wall time around calls that end in a device synchronise (both download x). Both must give
identical bits (x, f, |g|, iterations), or the exit status is 1.

usage: python tools/bench_batch.py [--n 10000] [--m 5] [--iters 300] [--reps 2] [--batches 1,16,256,1024] [out.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-lbfgs_amd"))
import lbfgs_amd as L  # noqa: E402
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000)
ap.add_argument("--m", type=int, default=5)
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--batches", default="1,16,256,1024")
ap.add_argument("--ls", default="backtracking")
ap.add_argument("out", nargs="?")
a = ap.parse_args()
OBJ, TOL = "rosenbrock", 0.0
batches = [int(b) for b in a.batches.split(",")]
X_all = np.stack([L.x0_uniform(a.n, p + 1, -2.0, 2.0) for p in range(max(batches))])


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


rows, ok = [], True
with L.Context(a.n, a.m) as ctx:
    for B in batches:
        X0 = np.ascontiguousarray(X_all[:B])
        with L.Batch(a.n, a.m, B) as bt:
            bt.minimize(OBJ, X0, a.ls, max_iterations=20, tolerance=TOL)  # warm-up: code objects, first launches
            ctx.minimize(OBJ, X0[0], a.ls, max_iterations=20, tolerance=TOL)
            out_b, out_1 = np.zeros_like(X0), np.zeros(a.n)
            for rep in range(a.reps):
                t = time.perf_counter()
                rb = bt.minimize(OBJ, X0, a.ls, max_iterations=a.iters, tolerance=TOL, out=out_b)
                t_batch = time.perf_counter() - t
                xs, fs, gs, its = [], [], [], []
                t = time.perf_counter()
                for p in range(B):
                    r1 = ctx.minimize(OBJ, X0[p], a.ls, max_iterations=a.iters, tolerance=TOL, out=out_1)
                    xs.append(out_1.copy())
                    fs.append(r1["f"])
                    gs.append(r1["gnorm"])
                    its.append(r1["iterations"])
                t_loop = time.perf_counter() - t
                same = (np.array_equal(bits(rb["x"]), bits(np.stack(xs))) and np.array_equal(bits(rb["f"]), bits(fs))
                        and np.array_equal(bits(rb["gnorm"]), bits(gs)) and list(rb["iterations"]) == its)
                ok &= same
                total = int(sum(its))
                row = dict(n=a.n, m=a.m, ls=a.ls, B=B, rep=rep, iterations_total=total,
                           batch_s=t_batch, loop_s=t_loop, batch_it_per_s=total / t_batch, loop_it_per_s=total / t_loop,
                           ratio=t_loop / t_batch, launches=rb["launches"], identical_bits=bool(same))
                rows.append(row)
                print(f"B={B:5d} rep={rep}: batch {row['batch_it_per_s']:12.0f} it/s ({t_batch * 1e3:9.2f} ms)   "
                      f"loop {row['loop_it_per_s']:10.0f} it/s ({t_loop * 1e3:9.2f} ms)   batch/loop {row['ratio']:7.2f}x   "
                      f"identical bits: {same}", flush=True)
if a.out:
    with open(a.out, "w") as fp:
        json.dump(dict(tool="tools/bench_batch.py", objective=OBJ, tolerance=TOL, iters=a.iters, rows=rows,
                       build=L.build_info()[0]), fp, indent=1)
sys.exit(0 if ok else 1)
