#!/usr/bin/env python3
"""Many small fits of a caller's torch model: one Batch with the batched callback against a loop of
single-problem solves, and the built-in objective as the floor.

The model is Rosenbrock written in torch, elementwise terms and f per row by sum(dim=1). Three routes
solve the same B problems (x0 = x0_uniform at seeds 10 + p) with the same iteration budget, tolerance
0 so that every problem spends it:
 (a) one Batch, Batch.set_device_objective(fn) with fn(Z, active) -> (F, G) over all rows at once, one
     call per round;
 (b) one Context, B times Context.minimize_device("device") with the same function on one row and
     eager_grad=True: one call, one stream synchronisation and a handful of launches per evaluation;
 (c) Batch.minimize("rosenbrock"), the library's own kernel: what no callback can beat.
(a) and (b) need not agree in bits (a row sum over a (B, n) tensor is not the sum of a vector of n);
iterations and evaluations are printed so that the work can be compared. Wall time is taken around
calls that end synchronised, each route after a warm-up, the routes alternating.

usage: python tools/bench_batch_callback.py [--cases 1000x16,1000x256,10000x16,10000x256] [--reps 2] [out.json]
"""
import argparse
import json
import os
import sys
import time

import torch  # before lbfgs_amd loads the library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import lbfgs_amd as L  # noqa: E402
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="1000x16,1000x256,10000x16,10000x256")
ap.add_argument("--m", type=int, default=5)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--ls", default="backtracking")
ap.add_argument("out", nargs="?")
a = ap.parse_args()
DEV = "cuda:0"


def rosenbrock_rows(Z, active):
    """every row at once (inactive rows cost nothing extra and are ignored)"""
    x, y = Z[:, :-1], Z[:, 1:]
    u = y - x * x
    F = (100.0 * u * u + (1.0 - x) * (1.0 - x)).sum(dim=1)
    G = torch.zeros(Z.shape, dtype=torch.float64, device=Z.device)
    G[:, :-1] = -400.0 * x * u - 2.0 * (1.0 - x)
    G[:, 1:] += 200.0 * u
    return F, G


def rosenbrock_row(x, want_grad):
    F, G = rosenbrock_rows(x.unsqueeze(0), None)
    return (F[0], G[0]) if want_grad else F[0]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


rows = []
for case in a.cases.split(","):
    n, B = (int(v) for v in case.split("x"))
    X0 = np.stack([L.x0_uniform(n, 10 + p, -2.0, 2.0) for p in range(B)])
    Xt = torch.from_numpy(X0).to(DEV)
    out = torch.empty((B, n), dtype=torch.float64, device=DEV)
    kw = dict(max_iterations=a.iters, tolerance=0.0)
    with L.Batch(n, a.m, B) as ba, L.Batch(n, a.m, B) as bc, L.Context(n, a.m) as c:
        ba.set_device_objective(rosenbrock_rows)
        c.set_device_objective(rosenbrock_row, eager_grad=True)

        def route_a(**k):
            return ba.minimize_device("device", Xt, a.ls, out=out, **dict(kw, **k))

        def route_b(count=B, **k):
            return [c.minimize_device("device", Xt[p], a.ls, out=out[p], **dict(kw, **k)) for p in range(count)]

        def route_c(**k):
            return bc.minimize_device("rosenbrock", Xt, a.ls, out=out, **dict(kw, **k))

        route_a(max_iterations=3), route_b(2, max_iterations=3), route_c(max_iterations=3)  # warm-up
        for rep in range(a.reps):
            ta, ra = timed(route_a)
            tb, rb = timed(route_b)
            tc, rc = timed(route_c)
            row = dict(n=n, B=B, m=a.m, ls=a.ls, iteration_budget=a.iters, rep=rep,
                       batch_callback_s=ta, single_loop_s=tb, builtin_batch_s=tc, single_over_batch=tb / ta,
                       batch_callback_rounds=int(ra["launches"]) - 1, batch_callback_launches=int(ra["launches"]),
                       batch_callback_evaluations=int(np.sum(ra["f_calls"])),
                       batch_callback_iterations=int(np.sum(ra["iterations"])),
                       single_loop_evaluations=int(sum(r["grad_calls"] for r in rb)),
                       single_loop_iterations=int(sum(r["iterations"] for r in rb)),
                       builtin_batch_iterations=int(np.sum(rc["iterations"])))
            rows.append(row)
            print(json.dumps(row), flush=True)
    del Xt, out
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(dict(tool="tools/bench_batch_callback.py", rows=rows, build=L.build_info()[0]), fp, indent=1)
