#!/usr/bin/env python3
"""A ragged batch against the routes a caller had without it, over the same problems in one process:

  ragged    one Batch(sizes, m).minimize over all B problems, the library's order of work (largest
            problems first) and, in a second object created under LBFGS_BATCH_ORDER=identity, the
            order 0, 1, 2, ...;
  by size   one uniform Batch per distinct size, created once outside the timing and solved one after
            another (the timing holds the solves only, not the gathering of each group's rows);
  loop      for B <= --loop-max and 16 distinct sizes, Context.minimize once per problem, one Context
            per distinct size created outside the timing (dense: with the problem's
            set_dense_quadratic inside it).

Problems: Rosenbrock (sizes from [32, 16384]) and dense quadratics (sizes from [8, 512], A symmetric
and diagonally dominant), m = 5, backtracking, a fixed iteration count (tolerance 0). The sizes are
B draws, with a fixed seed, from K distinct values, K in {16, 256}, for B in {256, 1024}. Wall time
around calls that end in a device synchronise, --reps repetitions after a warm-up of every route.
Every route must give identical bits (x, f, |g|, iterations) in every problem, or the exit status is 1.
No ratio is asserted.

usage: python tools/bench_batch_ragged.py [--reps 3] [--batches 256,1024] [--distinct 16,256] [--kinds rosenbrock,dense] [out.json]
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
ap.add_argument("--m", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", default="256,1024")
ap.add_argument("--distinct", default="16,256")
ap.add_argument("--kinds", default="rosenbrock,dense")
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--dense-iters", type=int, default=30)
ap.add_argument("--loop-max", type=int, default=256)
ap.add_argument("--ls", default="backtracking")
ap.add_argument("out", nargs="?")
a = ap.parse_args()
TOL = 0.0
RANGES = {"rosenbrock": (32, 16384), "dense": (8, 512)}


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def draw_sizes(kind, K, B):
    rs = np.random.RandomState(1000 * K + B)
    lo, hi = RANGES[kind]
    values = rs.choice(np.arange(lo, hi + 1), size=K, replace=False)
    return [int(v) for v in rs.choice(values, size=B)]


def dense_problem(n, seed):
    rs = np.random.RandomState(seed)
    R = rs.uniform(-1.0, 1.0, (n, n))
    return (R + R.T) / 2 + n * np.eye(n), rs.uniform(-1.0, 1.0, n)


def ragged_batch(sizes, identity):
    if identity:
        os.environ["LBFGS_BATCH_ORDER"] = "identity"  # read when the batch is created
    try:
        return L.Batch(sizes, a.m)
    finally:
        os.environ.pop("LBFGS_BATCH_ORDER", None)


def summary(res, B):
    return [res["x"][p] for p in range(B)], res["f"], res["gnorm"], list(res["iterations"])


def same(s1, s2):
    return (all(np.array_equal(bits(u), bits(v)) for u, v in zip(s1[0], s2[0])) and np.array_equal(bits(s1[1]), bits(s2[1]))
            and np.array_equal(bits(s1[2]), bits(s2[2])) and s1[3] == s2[3])


rows, ok = [], True
for kind in a.kinds.split(","):
    obj = "dense" if kind == "dense" else kind
    iters = a.dense_iters if kind == "dense" else a.iters
    for K in [int(v) for v in a.distinct.split(",")]:
        for B in [int(v) for v in a.batches.split(",")]:
            sizes = draw_sizes(kind, K, B)
            X0 = [L.x0_uniform(n, p + 1, -2.0, 2.0) for p, n in enumerate(sizes)]
            Ab = [dense_problem(n, p + 1) for p, n in enumerate(sizes)] if kind == "dense" else None
            groups = {}
            for p, n in enumerate(sizes):
                groups.setdefault(n, []).append(p)
            kw = dict(max_iterations=iters, tolerance=TOL)
            with ragged_batch(sizes, False) as rag, ragged_batch(sizes, True) as rag_id:
                uni = {n: L.Batch(n, a.m, len(ps)) for n, ps in groups.items()}
                uni_x0 = {n: np.stack([X0[p] for p in ps]) for n, ps in groups.items()}
                loop = B <= a.loop_max and K <= 16
                ctxs = {n: L.Context(n, a.m) for n in groups} if loop else {}
                if kind == "dense":
                    for bt in (rag, rag_id):
                        bt.set_dense_quadratics([q[0] for q in Ab], [q[1] for q in Ab])
                    for n, ps in groups.items():
                        uni[n].set_dense_quadratics(np.stack([Ab[p][0] for p in ps]), np.stack([Ab[p][1] for p in ps]))

                def run_ragged(bt):
                    t = time.perf_counter()
                    r = bt.minimize(obj, X0, a.ls, **kw)
                    return time.perf_counter() - t, summary(r, B)

                def run_by_size():
                    res = {}
                    t = time.perf_counter()
                    for n in groups:
                        res[n] = uni[n].minimize(obj, uni_x0[n], a.ls, **kw)
                    dt = time.perf_counter() - t
                    xs, fs, gs, its = [None] * B, np.zeros(B), np.zeros(B), [0] * B
                    for n, ps in groups.items():
                        for i, p in enumerate(ps):
                            xs[p], fs[p], gs[p], its[p] = res[n]["x"][i], res[n]["f"][i], res[n]["gnorm"][i], int(res[n]["iterations"][i])
                    return dt, (xs, fs, gs, its)

                def run_loop():
                    xs, fs, gs, its = [], np.zeros(B), np.zeros(B), []
                    t = time.perf_counter()
                    for p, n in enumerate(sizes):
                        if kind == "dense":
                            ctxs[n].set_dense_quadratic(*Ab[p])
                        r = ctxs[n].minimize(obj, X0[p], a.ls, **kw)
                        xs.append(r["x"])
                        fs[p], gs[p] = r["f"], r["gnorm"]
                        its.append(int(r["iterations"]))
                    return time.perf_counter() - t, (xs, fs, gs, its)

                routes = [("ragged", lambda: run_ragged(rag)), ("ragged_identity", lambda: run_ragged(rag_id)),
                          ("by_size", run_by_size)] + ([("loop", run_loop)] if loop else [])
                for _, fn in routes:  # warm-up: code objects, first launches
                    fn()
                for rep in range(a.reps):
                    times, ref = {}, None
                    for name, fn in routes:
                        times[name], s = fn()
                        if ref is None:
                            ref = s
                        elif not same(ref, s):
                            ok = False
                            times[name + "_differs"] = True
                    total = int(sum(ref[3]))
                    row = dict(kind=kind, distinct=K, distinct_drawn=len(groups), B=B, rep=rep, m=a.m, ls=a.ls, iters=iters,
                               n_min=min(sizes), n_max=max(sizes), n_sum=int(sum(sizes)), iterations_total=total,
                               identical_bits=not any(k.endswith("_differs") for k in times),
                               **{k + "_s": v for k, v in times.items() if not k.endswith("_differs")})
                    rows.append(row)
                    print(f"{kind:10s} K={K:3d} B={B:5d} rep={rep}: " +
                          "  ".join(f"{k} {v * 1e3:9.2f} ms" for k, v in times.items() if not k.endswith("_differs")) +
                          f"  identical bits: {row['identical_bits']}", flush=True)
                for bt in uni.values():
                    bt.close()
                for c in ctxs.values():
                    c.close()
if a.out:
    with open(a.out, "w") as fp:
        json.dump(dict(tool="tools/bench_batch_ragged.py", tolerance=TOL, rows=rows, build=L.build_info()[0]), fp, indent=1)
sys.exit(0 if ok else 1)
