#!/usr/bin/env python3
"""Batched dense quadratics against a loop of single solves: wall time of one Batch.minimize("dense")
over B problems with their own A and b, and of Context.set_dense_quadratic + Context.minimize("dense")
called once per problem, the same problems in the same process. The problems are the known-answer
data of tests/golden/matrices.npz: A_p = mat_n + 0.25 (p mod 16) I, b_p = (1 + p mod 16) linear_n,
x0 = x0_uniform(n, 10 + p, -2, 2); m = 5, backtracking, tolerance 1e-5, so every problem converges
(25 to 60 iterations at n = 500). The two alternate after a warm-up of both; wall time around calls
that end in a device synchronise. The loop's time includes its per-problem upload of A (it has no
other way to change the data); the batch's upload (Batch.set_dense_quadratics, once for all
problems) is timed separately and reported beside its solve. Both must give identical bits (x, f,
|g|, iterations, trials, commits), or the exit status is 1.

usage: python tools/bench_batch_dense.py [--cases 100x256,500x256,500x1024,500x256s] [--reps 3] [out.json]
       (a trailing s: one matrix shared by every problem)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import lbfgs_amd as L  # noqa: E402
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="100x256,500x256,500x1024,500x256s")
ap.add_argument("--m", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ls", default="backtracking")
ap.add_argument("out", nargs="?")
a = ap.parse_args()
TOL, MAXIT = 1e-5, 1000
data = np.load(os.path.join(ROOT, "tests", "golden", "matrices.npz"), allow_pickle=False)


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def problems(n, B, shared):
    q = np.arange(B) % 16
    mat, lin = data[f"mat{n}"], data[f"linear{n}"]
    b = (1.0 + q)[:, None] * lin[None, :]
    X0 = np.stack([L.x0_uniform(n, 10 + p, -2.0, 2.0) for p in range(B)])
    if shared:
        return np.ascontiguousarray(mat), b, X0
    A = np.empty((B, n, n))
    A[:] = mat
    i = np.arange(n)
    A[:, i, i] += 0.25 * q[:, None]
    return A, b, X0


rows, ok = [], True
for case in a.cases.split(","):
    shared = case.endswith("s")
    n, B = (int(v) for v in case.rstrip("s").split("x"))
    A, b, X0 = problems(n, B, shared)
    with L.Context(n, a.m) as ctx, L.Batch(n, a.m, B) as bt:
        bt.set_dense_quadratics(A, b)  # warm-up of both: code objects, allocations, first launches
        bt.minimize("dense", X0, a.ls, max_iterations=3, tolerance=TOL)
        ctx.set_dense_quadratic(A if shared else A[0], b[0])
        ctx.minimize("dense", X0[0], a.ls, max_iterations=3, tolerance=TOL)
        out_b, out_1 = np.zeros_like(X0), np.zeros(n)
        for rep in range(a.reps):
            t = time.perf_counter()
            bt.set_dense_quadratics(A, b)
            t_set = time.perf_counter() - t
            t = time.perf_counter()
            rb = bt.minimize("dense", X0, a.ls, max_iterations=MAXIT, tolerance=TOL, out=out_b)
            t_batch = time.perf_counter() - t
            xs, cols = [], {k: [] for k in ("f", "gnorm", "iterations", "trials_f", "trials_fg", "commits")}
            t = time.perf_counter()
            for p in range(B):
                ctx.set_dense_quadratic(A if shared else A[p], b[p])
                r1 = ctx.minimize("dense", X0[p], a.ls, max_iterations=MAXIT, tolerance=TOL, out=out_1)
                xs.append(out_1.copy())
                for k in cols:
                    cols[k].append(r1[k])
            t_loop = time.perf_counter() - t
            same = np.array_equal(bits(rb["x"]), bits(np.stack(xs))) and all(
                np.array_equal(bits(np.asarray(rb[k], np.float64)), bits(np.asarray(cols[k], np.float64))) for k in cols)
            ok &= bool(same)
            total = int(sum(cols["iterations"]))
            row = dict(n=n, m=a.m, ls=a.ls, B=B, shared_A=shared, rep=rep, iterations_total=total,
                       iterations_min=int(min(cols["iterations"])), iterations_max=int(max(cols["iterations"])),
                       batch_set_s=t_set, batch_solve_s=t_batch, loop_s=t_loop,
                       ratio_solve=t_loop / t_batch, ratio_with_upload=t_loop / (t_batch + t_set),
                       launches=rb["launches"], bytes_per_problem_mean=float(np.mean(rb["bytes"])),
                       identical_bits=bool(same))
            rows.append(row)
            print(f"n={n:4d} B={B:5d}{' shared' if shared else '       '} rep={rep}: batch {t_batch * 1e3:9.2f} ms "
                  f"(+ upload {t_set * 1e3:8.2f} ms)   loop {t_loop * 1e3:10.2f} ms   loop/batch {row['ratio_solve']:7.2f}x "
                  f"(with upload {row['ratio_with_upload']:6.2f}x)   {total} iterations   identical bits: {same}", flush=True)
    del A
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(dict(tool="tools/bench_batch_dense.py", tolerance=TOL, max_iterations=MAXIT, rows=rows,
                       build=L.build_info()[0]), fp, indent=1)
sys.exit(0 if ok else 1)
