#!/usr/bin/env python3
"""Batched dense quadratics whose A, b and X0 are CUDA tensors: the host route against the device route.

Route H (all there was before the device forms): the tensors go to numpy, Batch.set_dense_quadratics
copies A and b back to the device into the batch's own store, Batch.minimize uploads x0 and downloads
x, and the result goes back into a tensor. Route D: Batch.set_dense_quadratics_device (by reference,
nothing copied) and Batch.minimize_device (the kernel reads and writes the tensors' rows). The
problems are tools/bench_batch_dense.py's four cases (the known-answer data of
tests/golden/matrices.npz, m = 5, backtracking, tolerance 1e-5), and one more row whose matrices have
the row stride n + 1. Each route has its own Batch object; the two alternate after a warm-up of both,
wall time around calls that end in a device synchronise, setter and solve timed separately. The device
memory a route's first setter call takes is read from torch.cuda.mem_get_info around it and printed
beside plan_dense - plan. Both routes must give identical bits (x, f, |g|, iterations, trials,
commits), or the exit status is 1.

usage: python tools/bench_batch_device.py [--cases 100x256,500x256,500x1024,500x256s,500x256p] [--reps 3] [out.json]
       (a trailing s: one matrix shared by every problem; a trailing p: row stride n + 1)
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
ap.add_argument("--cases", default="100x256,500x256,500x1024,500x256s,500x256p")
ap.add_argument("--m", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ls", default="backtracking")
ap.add_argument("out", nargs="?")
a = ap.parse_args()
TOL, MAXIT, DEV = 1e-5, 1000, "cuda:0"
KEYS = ("f", "gnorm", "iterations", "trials_f", "trials_fg", "commits")
data = np.load(os.path.join(ROOT, "tests", "golden", "matrices.npz"), allow_pickle=False)


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def problems(n, B, shared):  # tools/bench_batch_dense.py's
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


def timed(fn):
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def taken(fn):
    """device bytes that fn() takes and keeps"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    fn()
    torch.cuda.synchronize()
    return free0 - torch.cuda.mem_get_info()[0]


rows, ok = [], True
for case in a.cases.split(","):
    shared, padded = case.endswith("s"), case.endswith("p")
    n, B = (int(v) for v in case.rstrip("sp").split("x"))
    A, b, X0 = problems(n, B, shared)
    if padded:
        At = torch.zeros((B, n, n + 1), dtype=torch.float64, device=DEV)[:, :, :n]
        At.copy_(torch.from_numpy(A))
    else:
        At = torch.from_numpy(A).to(DEV)
    bt_, Xt = torch.from_numpy(b).to(DEV), torch.from_numpy(X0).to(DEV)
    del A, b, X0
    lda = At.stride(-2)
    out_h, out_d = np.zeros((B, n)), torch.empty((B, n), dtype=torch.float64, device=DEV)

    def route_h(bh, maxit=MAXIT):
        t_set, _ = timed(lambda: bh.set_dense_quadratics(At.cpu().numpy(), bt_.cpu().numpy()))
        t_solve, r = timed(lambda: (lambda res: (res, torch.from_numpy(res["x"]).to(DEV)))(
            bh.minimize("dense", Xt.cpu().numpy(), a.ls, max_iterations=maxit, tolerance=TOL, out=out_h)))
        return t_set, t_solve, r[0], r[1]

    def route_d(bd, maxit=MAXIT):
        t_set, _ = timed(lambda: bd.set_dense_quadratics_device(At, bt_))
        t_solve, r = timed(lambda: bd.minimize_device("dense", Xt, a.ls, max_iterations=maxit, tolerance=TOL, out=out_d))
        return t_set, t_solve, r, r["x"]

    with L.Batch(n, a.m, B) as bh, L.Batch(n, a.m, B) as bd:
        # warm-up of both, and what each route's first setter call takes
        mem_h = taken(lambda: bh.set_dense_quadratics(At.cpu().numpy(), bt_.cpu().numpy()))
        mem_d = taken(lambda: bd.set_dense_quadratics_device(At, bt_))
        route_h(bh, 3)
        route_d(bd, 3)
        plan = L.plan_dense(n, a.m, B, shared) - L.plan(n, a.m, B)
        for rep in range(a.reps):
            hs, hv, rh, xh = route_h(bh)
            ds, dv, rd, xd = route_d(bd)
            same = bool(torch.equal(xh.view(torch.int64), xd.view(torch.int64))) and all(
                np.array_equal(bits(np.asarray(rh[k], np.float64)), bits(np.asarray(rd[k], np.float64))) for k in KEYS)
            ok &= same
            row = dict(n=n, m=a.m, ls=a.ls, B=B, shared_A=shared, lda=lda, rep=rep,
                       iterations_total=int(np.sum(rd["iterations"])), host_set_s=hs, host_solve_s=hv, device_set_s=ds,
                       device_solve_s=dv, ratio_end_to_end=(hs + hv) / (ds + dv), host_setter_bytes=mem_h,
                       device_setter_bytes=mem_d, plan_dense_minus_plan=plan, identical_bits=same)
            rows.append(row)
            print(f"n={n:4d} B={B:5d} lda={lda:4d}{' shared' if shared else '       '} rep={rep}: "
                  f"H set {hs * 1e3:8.2f} + solve {hv * 1e3:8.2f} ms   D set {ds * 1e3:6.2f} + solve {dv * 1e3:8.2f} ms   "
                  f"H/D {row['ratio_end_to_end']:5.2f}x   setter takes H {mem_h / 2**20:8.1f} MiB, D {mem_d / 2**20:6.1f} MiB "
                  f"(plan_dense - plan {plan / 2**20:8.1f} MiB)   identical bits: {same}", flush=True)
    del At, bt_, Xt, out_d
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(dict(tool="tools/bench_batch_device.py", tolerance=TOL, max_iterations=MAXIT, rows=rows,
                       build=L.build_info()[0]), fp, indent=1)
sys.exit(0 if ok else 1)
