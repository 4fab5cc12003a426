#!/usr/bin/env python3
"""Measurements for the device-callback objective, the device-buffer entry points and the reducer
(DESIGN.md §4.7). Three steps, each a process of its own under its own time limit, one at a time;
each writes profiles/devobj/<step>.json and prints it.

  callback  a torch Rosenbrock (elementwise terms, f through Reducer.sum) at n = 1e7, m = 10,
            backtracking: ms per iteration over 20 iterations after a history fill of m, through
            LBFGS_OBJ_DEVICE without and with eager_grad, through LBFGS_OBJ_HOST (the same callable,
            x to the GPU and f / g back per call) and the built-in LBFGS_OBJ_ROSENBROCK
  buffers   configs[3]'s shape (tridiagonal quadratic n = 1e8, m = 20, Wolfe, to tol 1e-5): time to
            solution through minimize_device (x0 and x resident) and through minimize (host buffers)
  reducer   Reducer.dot at n = 1e8 in GB/s, aligned and one-element-offset buffers, beside k_dot's
            event-timed rate (lbfgs_prof_get(LBFGS_KERNEL_DOT)) in the same process

usage: python tools/bench_device_objective.py [--steps callback,buffers,reducer] [--out DIR]
       (--step NAME runs that step in this process; --n scales a step down for a quick look)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"callback": 420, "buffers": 300, "reducer": 240}  # seconds per step


def _load():
    import torch  # before the library: one HIP runtime for both (lbfgs_amd._torch)

    sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
    import lbfgs_amd as L

    return torch, L


def torch_rosenbrock(torch, red):
    def fn(x, want_grad):
        a, b = x[:-1], x[1:]
        u = b - a * a
        t = torch.zeros_like(x)
        t[:-1] = 100.0 * u * u + (1.0 - a) * (1.0 - a)
        f = red.sum(t)
        if not want_grad:
            return f
        g = torch.zeros_like(x)
        g[:-1] = -400.0 * a * u - 2.0 * (1.0 - a)
        g[1:] += 200.0 * u
        return f, g

    return fn


def step_callback(n):
    import ctypes as C

    import numpy as np

    torch, L = _load()
    n = n or 10 ** 7
    m, fill, iters, ls = 10, 10, 20, "backtracking"
    x0 = L.x0_uniform(n, 42, -2.0, 2.0)
    t0 = torch.from_numpy(x0).to("cuda:0")
    res = dict(step="callback", n=n, m=m, line_search=ls, fill=fill, iterations=iters, build=L.build_info()[0],
               torch=torch.__version__)

    def timed(c):
        c.step(fill)
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = c.step(iters)
        c.sync()
        dt = time.perf_counter() - t
        return dict(ms_per_iteration=1e3 * dt / iters, f=r["f"], f_calls=r["f_calls"], grad_calls=r["grad_calls"],
                    status=r["status"])

    with L.Reducer(n) as red, L.Context(n, m) as c:
        fn = torch_rosenbrock(torch, red)
        for name, eager in (("device", False), ("device_eager_grad", True)):
            c.set_device_objective(fn, eager_grad=eager)
            c.init_device("device", t0, ls)
            res[name] = timed(c)
            print(name, json.dumps(res[name]), flush=True)
        # the same callable through the host-callback path
        to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
        cb = c._host_fn(lambda x: fn(to_dev(x), False), lambda x: fn(to_dev(x), True)[1].cpu().numpy())
        k = L.constants()
        rc = L.lib().lbfgs_solver_init(c.h, L.OBJECTIVES["host"], C.byref(cb), L.LINE_SEARCHES[ls], C.byref(k), x0,
                                       1e-5, L.FLAG_QUIET)
        assert rc == 0, rc
        res["host"] = timed(c)
        print("host", json.dumps(res["host"]), flush=True)
        c.init_device("rosenbrock", t0, ls)
        res["builtin_rosenbrock"] = timed(c)
        print("builtin", json.dumps(res["builtin_rosenbrock"]), flush=True)
    res["device_over_host"] = res["host"]["ms_per_iteration"] / res["device"]["ms_per_iteration"]
    return res


def step_buffers(n):
    import numpy as np

    torch, L = _load()
    n = n or 10 ** 8
    m, ls = 20, "wolfe"
    x0 = L.x0_uniform(n, 42, -2.0, 2.0)
    t0 = torch.from_numpy(x0).to("cuda:0")
    tx = torch.empty_like(t0)
    xh = np.zeros(n)
    res = dict(step="buffers", config="configs[3]: quad_tridiag n=%d m=%d %s, tol 1e-5" % (n, m, ls),
               build=L.build_info()[0])
    with L.Context(n, m) as c:
        for rep in range(3):  # the first pass of each form also pays first touches
            torch.cuda.synchronize()
            t = time.perf_counter()
            rd = c.minimize_device("quad_tridiag", t0, ls, 1000, out=tx)
            td = time.perf_counter() - t
            t = time.perf_counter()
            rh = c.minimize("quad_tridiag", x0, ls, 1000, out=xh)
            th = time.perf_counter() - t
            same = bool(np.array_equal(tx.cpu().numpy().view(np.uint64), xh.view(np.uint64)))
            res["rep%d" % rep] = dict(device_buffers_ms=1e3 * td, host_buffers_ms=1e3 * th,
                                      device_solver_ms=1e3 * rd["seconds"], host_solver_ms=1e3 * rh["seconds"],
                                      iterations=rd["iterations"], status=rd["status"], same_bits=same)
            print(json.dumps(res["rep%d" % rep]), flush=True)
    return res


def step_reducer(n):
    torch, L = _load()
    n = n or 10 ** 8
    reps = 20
    big_a = torch.empty(n + 2, dtype=torch.float64, device="cuda:0").uniform_(-2.0, 2.0)
    big_b = torch.empty(n + 2, dtype=torch.float64, device="cuda:0").uniform_(-2.0, 2.0)
    res = dict(step="reducer", n=n, reps=reps, build=L.build_info()[0])
    with L.Reducer(n) as red:
        for name, off in (("aligned16", 0), ("offset_one_element", 1)):
            a, b = big_a[off:off + n], big_b[off:off + n]
            red.dot(a, b)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                v = red.dot(a, b)
            dt = (time.perf_counter() - t) / reps
            res[name] = dict(us=1e6 * dt, gbps=16.0 * n / dt / 1e9, value=v)
            t = time.perf_counter()
            for _ in range(reps):
                v = red.sum(a)
            dt = (time.perf_counter() - t) / reps
            res[name + "_sum"] = dict(us=1e6 * dt, gbps=8.0 * n / dt / 1e9, value=v)
            print(name, json.dumps(res[name]), json.dumps(res[name + "_sum"]), flush=True)
    # k_dot on the solver's padded vectors, event-timed, same process (host-timed wall beside it
    # would include two 800 MB uploads)
    ah = big_a[:n].cpu().numpy()
    with L.Context(n, 1) as c:
        c.prof_enable(True)
        c.dot(ah, ah)
        c.prof_reset()
        for _ in range(5):
            v = c.dot(ah, ah)
        p = c.prof_get("dot")
        res["k_dot"] = dict(us=1e3 * p["ms"] / max(p["launches"], 1), launches=p["launches"],
                            gbps=p["bytes"] / (p["ms"] * 1e-3) / 1e9 if p["ms"] > 0 else None, value=v)
        g = c.prof_get("group_reduce")
        res["k_dot_stage2_us"] = 1e3 * g["ms"] / max(g["launches"], 1)
    res["same_bits_as_context_dot"] = red_equal(L, torch, big_a[:n], ah, n)
    print("k_dot", json.dumps(res["k_dot"]), flush=True)
    return res


def red_equal(L, torch, a, ah, n):
    import numpy as np

    with L.Reducer(n) as red, L.Context(n, 1) as c:
        return bool(np.float64(red.dot(a, a)).view(np.uint64) == np.float64(c.dot(ah, ah)).view(np.uint64))


STEPS = {"callback": step_callback, "buffers": step_buffers, "reducer": step_reducer}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="callback,buffers,reducer")
    ap.add_argument("--step", default=None)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "devobj"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        res = STEPS[a.step](a.n)
        with open(os.path.join(a.out, a.step + ".json"), "w") as fp:
            json.dump(res, fp, indent=1)
        print(json.dumps(res), flush=True)
        return 0
    for s in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[s]), sys.executable, os.path.abspath(__file__), "--step", s,
               "--out", a.out] + (["--n", str(a.n)] if a.n else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:  # nothing more is started on the GPU after a step that failed or ran out of time
            print(f"step {s} ended with {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
