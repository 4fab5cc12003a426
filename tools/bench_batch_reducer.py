#!/usr/bin/env python3
"""What f costs a batch callback: the canonical row sums in one launch (reduce_rows) against a loop of
single-vector reductions (Reducer.sum, one per row) and torch's own sum(dim=1), which is not canonical
and is the floor.

For every case n x B, twice:
 1. time per call of (a) reduce_rows(T), (b) B times Reducer.sum(T[p]), (c) torch.sum(T, dim=1) on a
    (B, n) table of uniform(-2, 2) values: stream events around 200 back-to-back calls (for (b) the
    host waits between its launches are inside the bracket, as they are for a caller), and the host
    clock around the same calls, ending synchronised;
 2. the whole batched-callback solve of tools/bench_batch_callback.py (Rosenbrock in torch, m = 5,
    backtracking, 30 iterations, tolerance 0: every problem spends the budget) with f formed by each
    of (a), (b), (c). (b) brings the mask to the host and reduces the active rows, as
    tests/batchcb_gpu_cases.py::per_row does. Wall time around calls that end synchronised, each route
    after a warm-up, the routes alternating.
(a) and (b) give the same bits (checked: `same_bits`), (c) need not; the rounds are printed so that the
work can be compared.

Every case runs in a child process under its own time limit; the first failure stops the run. The
parent touches no GPU.

usage: python tools/bench_batch_reducer.py [--cases 1000x16,1000x256,10000x16,10000x256] [--reps 2]
                                           [--limit 300] [out-prefix]
writes <out-prefix>.txt (one JSON line per case and repetition) and <out-prefix>.json; the default
prefix is profiles/batch_reducer/bench_batch_reducer
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="1000x16,1000x256,10000x16,10000x256")
ap.add_argument("--m", type=int, default=5)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--ls", default="backtracking")
ap.add_argument("--limit", type=int, default=300, help="seconds a case's child process may take")
ap.add_argument("--child", help="(internal) run this one case, NxB, and print its JSON lines")
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "batch_reducer", "bench_batch_reducer"))
a = ap.parse_args()


def parent():
    rows, build = [], None
    for case in a.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--m", str(a.m), "--iters", str(a.iters),
               "--reps", str(a.reps), "--calls", str(a.calls), "--ls", a.ls]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(f"case {case}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"case {case}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", file=sys.stderr)
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                row = json.loads(line)
                build = row.pop("build", build)
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".txt", "w") as fp:
        for row in rows:
            fp.write(json.dumps(row) + "\n")
    with open(a.out + ".json", "w") as fp:
        json.dump(dict(tool="tools/bench_batch_reducer.py", rows=rows, build=build), fp, indent=1)
    return 0


def child():
    import torch  # before lbfgs_amd loads the library: one HIP runtime for both

    sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
    import lbfgs_amd as L
    import numpy as np

    DEV = "cuda:0"
    n, B = (int(v) for v in a.child.split("x"))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    def per_call(fn):
        """(microseconds per call by stream events, by the host clock) over a.calls back-to-back calls"""
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        wall = time.perf_counter() - t
        return e0.elapsed_time(e1) * 1e3 / a.calls, wall * 1e6 / a.calls

    def terms(Z):
        x, y = Z[:, :-1], Z[:, 1:]
        u = y - x * x
        T = torch.zeros(Z.shape, dtype=torch.float64, device=Z.device)
        T[:, :-1] = 100.0 * u * u + (1.0 - x) * (1.0 - x)
        G = torch.zeros(Z.shape, dtype=torch.float64, device=Z.device)
        G[:, :-1] = -400.0 * x * u - 2.0 * (1.0 - x)
        G[:, 1:] += 200.0 * u
        return T, G

    with L.Reducer(n) as red, L.Batch(n, a.m, B) as ba, L.Batch(n, a.m, B) as bb, L.Batch(n, a.m, B) as bc:
        def f_rows(Z, active):
            T, G = terms(Z)
            return L.reduce_rows(T, active=active), G

        def f_loop(Z, active):
            T, G = terms(Z)
            F = torch.full((B,), float("nan"), dtype=torch.float64, device=Z.device)
            for p in np.flatnonzero(active.cpu().numpy()):
                F[p] = red.sum(T[p])
            return F, G

        def f_torch(Z, active):
            T, G = terms(Z)
            return T.sum(dim=1), G

        rng = np.random.default_rng(n + B)
        T = torch.from_numpy(rng.uniform(-2.0, 2.0, (B, n))).to(DEV)
        out = torch.empty(B, dtype=torch.float64, device=DEV)
        loop = [red.sum(T[p]) for p in range(B)]
        same = bool(np.array_equal(np.array(loop).view(np.uint64), L.reduce_rows(T).cpu().numpy().view(np.uint64)))

        X0 = np.stack([L.x0_uniform(n, 10 + p, -2.0, 2.0) for p in range(B)])
        Xt = torch.from_numpy(X0).to(DEV)
        X = torch.empty((B, n), dtype=torch.float64, device=DEV)
        kw = dict(max_iterations=a.iters, tolerance=0.0)
        routes = []
        for b, fn in ((ba, f_rows), (bb, f_loop), (bc, f_torch)):
            b.set_device_objective(fn)
            routes.append(lambda b=b, **k: b.minimize_device("device", Xt, a.ls, out=X, **dict(kw, **k)))
        for r in routes:
            r(max_iterations=3)  # warm-up
        for rep in range(a.reps):
            ca = per_call(lambda: L.reduce_rows(T, out=out))
            cb = per_call(lambda: [red.sum(T[p]) for p in range(B)])
            cc = per_call(lambda: torch.sum(T, dim=1, out=out))
            (ta, ra), (tb, rb), (tc, rc) = (timed(r) for r in routes)
            fa, fb = np.array(ra["f"]), np.array(rb["f"])
            row = dict(n=n, B=B, m=a.m, ls=a.ls, iteration_budget=a.iters, rep=rep, calls=a.calls,
                       call_us_reduce_rows=ca[0], call_us_reducer_loop=cb[0], call_us_torch_sum=cc[0],
                       call_wall_us_reduce_rows=ca[1], call_wall_us_reducer_loop=cb[1], call_wall_us_torch_sum=cc[1],
                       loop_over_rows_per_call=cb[0] / ca[0], same_bits=same,
                       solve_s_reduce_rows=ta, solve_s_reducer_loop=tb, solve_s_torch_sum=tc,
                       solve_loop_over_rows=tb / ta, solve_rows_over_torch=ta / tc,
                       rounds_reduce_rows=int(ra["launches"]) - 1, rounds_reducer_loop=int(rb["launches"]) - 1,
                       rounds_torch_sum=int(rc["launches"]) - 1,
                       solve_same_bits=bool(np.array_equal(fa.view(np.uint64), fb.view(np.uint64))),
                       build=L.build_info()[0])
            print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(child() if a.child else parent())
