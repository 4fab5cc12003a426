"""The GPU cases of tests/test_gpu_device_objective.py, which runs this file in a process of its own
(see there: torch is imported before the library is loaded, so that both use one HIP runtime).

Device-callback objectives (LBFGS_OBJ_DEVICE), device-resident x0 / x, and the canonical
reductions on caller-owned buffers (lbfgs_reducer_*). Everything compares bits.

1. the device callback against the oracle and against the host-callback path, call counts included,
   also with line-search constants that are not the defaults (tests/consts_cases.py, path 11);
2. real device math: torch objectives reduced through Reducer.sum, LBFGS_OBJ_DEVICE against the same
   torch function through LBFGS_OBJ_HOST;
3. minimize_device / init_device / get_x_device against the host-buffer forms, on slices at storage
   offset 1 of sentinel-filled allocations;
4. the refusals, a failing callback, a Python exception;
5. Reducer.dot / .sum against the oracle's canonical order and Context.dot, on aligned and
   one-element-offset buffers between NaN sentinels.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  before lbfgs_amd loads liblbfgs_hip.so: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import consts_cases as K  # noqa: E402
import lbfgs_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import test_gpu_host_callbacks as H  # noqa: E402  (its CASES and its Log callables)

pytestmark = pytest.mark.gpu

BAD_ARG, ERR_CALLBACK = -1, -6
SENTINEL = 1234.5


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")


def same_alpha(a1, a2):
    return np.array_equal(np.isnan(a1), np.isnan(a2)) and np.array_equal(a1[~np.isnan(a1)], a2[~np.isnan(a2)])


def same_run(r, s, keys=("tr_f", "tr_gnorm")):
    """two runs of the binding: x, traces, result fields and messages, bit for bit"""
    assert np.array_equal(bits(host(r["x"]) if hasattr(r["x"], "cpu") else r["x"]),
                          bits(host(s["x"]) if hasattr(s["x"], "cpu") else s["x"]))
    for key in keys:
        assert np.array_equal(bits(r[key]), bits(s[key])), key
    assert same_alpha(r["tr_alpha"], s["tr_alpha"])
    for key in ("iterations", "status", "trials_f", "trials_fg", "commits", "h_min", "h_max", "messages"):
        assert r[key] == s[key], key
    assert bits([r["f"]])[0] == bits([s["f"]])[0] and bits([r["gnorm"]])[0] == bits([s["gnorm"]])[0]


# ---- 1. against the oracle ---------------------------------------------------------------------
class DeviceLog:
    """fn(x, want_grad) that brings x to the CPU and calls the oracle's f / grad (H.Log's callables)."""

    def __init__(self, obj):
        self.log = H.Log(obj)
        self.calls = []  # (want_grad, checksum of the point)

    def __call__(self, x, want_grad):
        xh = host(x)
        self.calls.append((bool(want_grad), O.np_checksum(xh)))
        f = self.log.f(xh)
        if not want_grad:
            return f
        return f, dev(self.log.grad(xh))


CASES1 = H.CASES + [("rosenbrock", 1, 1, "backtracking", 10), ("rosenbrock", 513, 3, "interpolation", 30)]


@pytest.mark.parametrize("obj,n,m,ls,iters", CASES1)
def test_device_callback_vs_oracle_and_host_path(obj, n, m, ls, iters):
    x0 = O.x0_uniform(n, 42, -2.0, 2.0)
    lo = H.Log(obj)
    o = O.lbfgs("host", x0, ls, m, iters, 1e-5, mode=O.CANON, f=lo.f, grad=lo.grad)
    lh = H.Log(obj)
    with L.Context(n, m) as c:
        rh = c.minimize("host", x0, ls, iters, f=lh.f, grad=lh.grad, trace=True)
        for eager in (False, True):
            d = DeviceLog(obj)
            c.set_device_objective(d, eager_grad=eager)
            r = c.minimize_device("device", dev(x0), ls, iters, trace=True)
            # the oracle
            assert np.array_equal(bits(host(r["x"])), bits(o["x"]))
            assert np.array_equal(bits(r["tr_f"]), bits(o["f"]))
            assert np.array_equal(bits(r["tr_gnorm"]), bits(o["gnorm"]))
            assert same_alpha(r["tr_alpha"], o["alpha"])
            assert r["iterations"] == o["iters"] and r["status"] == o["status"]
            assert r["messages"] == o["messages"]
            # the host-callback path in its default mode
            same_run(r, rh)
            pts = [k[1] for k in d.calls]
            if eager:
                assert all(k[0] for k in d.calls)          # every call carried a gradient
                assert len(pts) == len(set(pts))           # no point evaluated twice
                assert r["grad_calls"] == len(d.calls) and r["f_calls"] == rh["f_calls"]
            else:
                assert r["f_calls"] == rh["f_calls"] and r["grad_calls"] == rh["grad_calls"]
                assert r["grad_calls"] == sum(1 for k in d.calls if k[0])


# ---- 1b. line-search constants that are not the defaults (tests/consts_cases.py, path 11) --------
_host_runs = {}


def host_run(case):
    """the host-callback path's run of a case with its set's constants, computed once and shared"""
    if case not in _host_runs:
        ks, obj, n, m, ls, iters = case
        lh = H.Log(obj)
        with L.Context(n, m) as c:
            _host_runs[case] = c.minimize("host", K.oracle(case, host=True)["x0"], ls, iters, tolerance=K.TOL, f=lh.f,
                                          grad=lh.grad, trace=True, consts=K.device_constants(L, ks))
    return _host_runs[case]


@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
@pytest.mark.parametrize("case", K.DEVICE_OBJ, ids=lambda c: "-".join(str(v) for v in c))
def test_device_callback_with_varied_constants(case, eager):
    """K1 / K2 / K5 x the four searches through LBFGS_OBJ_DEVICE: the oracle's bits with the same
    constants, and the host-callback path's (tests/test_constants_inputs.py asserts on the CPU that
    the constants bite in these inputs)"""
    ks, obj, n, m, ls, iters = case
    o, rh = K.oracle(case, host=True), host_run(case)
    d = DeviceLog(obj)
    with L.Context(n, m) as c:
        c.set_device_objective(d, eager_grad=eager)
        r = c.minimize_device("device", dev(o["x0"]), ls, iters, K.TOL, trace=True, consts=K.device_constants(L, ks))
    assert np.array_equal(bits(host(r["x"])), bits(o["x"]))
    assert np.array_equal(bits(r["tr_f"]), bits(o["f"])) and np.array_equal(bits(r["tr_gnorm"]), bits(o["gnorm"]))
    assert same_alpha(r["tr_alpha"], o["alpha"])
    assert r["iterations"] == o["iters"] and r["status"] == o["status"] and r["messages"] == o["messages"]
    same_run(r, rh)
    assert len(d.calls) > 0 and r["f_calls"] == rh["f_calls"]
    if eager:
        assert all(k[0] for k in d.calls) and r["grad_calls"] == len(d.calls)
    else:
        assert r["grad_calls"] == rh["grad_calls"] == sum(1 for k in d.calls if k[0])


# ---- 2. real device math -----------------------------------------------------------------------
def torch_rosenbrock(red):
    """Rosenbrock with elementwise torch terms, f through the canonical reducer"""
    def fn(x, want_grad):
        n = x.numel()
        t = torch.zeros_like(x)
        g = torch.zeros_like(x)
        if n > 1:
            a, b = x[:-1], x[1:]
            u = b - a * a
            t[:-1] = 100.0 * u * u + (1.0 - a) * (1.0 - a)
            if want_grad:
                g[:-1] = -400.0 * a * u - 2.0 * (1.0 - a)
                g[1:] += 200.0 * u
        f = red.sum(t)
        return (f, g) if want_grad else f

    return fn


def torch_separable(red):
    def fn(x, want_grad):
        e = x - 1.0
        f = red.sum(e * e)
        return (f, 2.0 * e) if want_grad else f

    return fn


def through_host(fn):
    """the same torch function as LBFGS_OBJ_HOST callables: x to the GPU, f and g back"""
    return (lambda x: fn(dev(x), False)), (lambda x: host(fn(dev(x), True)[1]))


@pytest.mark.parametrize("make", [torch_rosenbrock, torch_separable])
@pytest.mark.parametrize("ls", ["wolfe", "backtracking"])
def test_torch_objective_device_vs_host_route(make, ls):
    n, m, iters = 2000, 5, 30
    x0 = O.x0_uniform(n, 42, -2.0, 2.0)
    with L.Reducer(n) as red, L.Context(n, m) as c:
        fn = make(red)
        f, grad = through_host(fn)
        rh = c.minimize("host", x0, ls, iters, f=f, grad=grad, trace=True)
        c.set_device_objective(fn)
        rd = c.minimize_device("device", dev(x0), ls, iters, trace=True)
        same_run(rd, rh)
        assert rd["grad_calls"] == rh["grad_calls"] and rd["iterations"] >= 2
        # the separable quadratic under Wolfe runs off to NaN steps (as in the reference), and at a NaN
        # step no point compares equal to the one f is known at: f rides along with the gradient again
        if np.all(np.isfinite(rh["tr_f"])):
            assert rd["f_calls"] == rh["f_calls"]
        else:
            assert rd["f_calls"] >= rh["f_calls"]
        c.set_device_objective(fn, eager_grad=True)
        same_run(c.minimize_device("device", dev(x0), ls, iters, trace=True), rh)


def test_torch_objective_on_a_side_stream():
    n, m, iters, ls = 2000, 5, 30, "wolfe"
    x0 = O.x0_uniform(n, 42, -2.0, 2.0)
    side = torch.cuda.Stream(device="cuda:0")
    with L.Reducer(n) as red, L.Context(n, m) as c:
        fn = torch_rosenbrock(red)

        def on_side(x, want_grad):
            with torch.cuda.stream(side):  # the reducer runs on the current stream: this one
                assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
                r = fn(x, want_grad)
            side.synchronize()  # the gradient is complete before the glue copies it
            return r

        f, grad = through_host(fn)
        rh = c.minimize("host", x0, ls, iters, f=f, grad=grad, trace=True)
        c.set_device_objective(on_side)
        same_run(c.minimize_device("device", dev(x0), ls, iters, trace=True), rh)


# ---- 3. device buffers ---------------------------------------------------------------------------
def sliced(n, values=None):
    """a tensor of n at storage offset 1 of a sentinel-filled allocation of n + 2"""
    big = torch.full((n + 2,), SENTINEL, dtype=torch.float64, device="cuda:0")
    t = big[1:n + 1]
    assert t.storage_offset() == 1 and t.is_contiguous()
    if values is not None:
        t.copy_(dev(values))
    return big, t


@pytest.mark.parametrize("n", [1, 5, 513, 10000, 70001])
@pytest.mark.parametrize("obj", ["rosenbrock", "quad_tridiag", "quad_sep"])
def test_minimize_device_equals_minimize(obj, n):
    m, iters, ls = 5, 12, "backtracking"
    assert n != 70001 or O.geometry(n)[0] == 2048
    x0 = O.x0_uniform(n, 42, -2.0, 2.0)
    big0, t0 = sliced(n, x0)
    bigx, tx = sliced(n)
    with L.Context(n, m) as c:
        rh = c.minimize(obj, x0, ls, iters, trace=True)
        rd = c.minimize_device(obj, t0, ls, iters, trace=True, out=tx)
        assert rd["x"] is tx
        same_run(rd, rh)
        assert np.array_equal(rd["tr_c1"], rh["tr_c1"]) and np.array_equal(rd["tr_c2"], rh["tr_c2"])
        assert rd["f_calls"] == rh["f_calls"] == 0 and rd["grad_calls"] == rh["grad_calls"] == 0
        # x0 unchanged, every sentinel intact
        assert np.array_equal(bits(host(t0)), bits(x0))
        for big in (big0, bigx):
            assert host(big[0]) == SENTINEL and host(big[n + 1]) == SENTINEL
        # a fresh result tensor as well
        assert np.array_equal(bits(host(c.minimize_device(obj, t0, ls, iters)["x"])), bits(rh["x"]))


@pytest.mark.parametrize("obj,n,ls", [("rosenbrock", 513, "wolfe"), ("quad_tridiag", 70001, "backtracking"),
                                      ("quad_sep", 5, "interpolation")])
def test_init_device_step_get_x_device(obj, n, ls):
    m = 5
    x0 = O.x0_uniform(n, 7, -2.0, 2.0)
    big0, t0 = sliced(n, x0)
    bigx, tx = sliced(n)
    with L.Context(n, m) as c:
        c.init(obj, x0, ls, trace=True)
        ra, rb = c.step(4), c.step(5)
        xh, th = c.get_x(), c.trace()
        c.init_device(obj, t0, ls, trace=True)
        da, db = c.step(4), c.step(5)
        xd, td = c.get_x_device(out=tx), c.trace()
        assert xd is tx
        for a, b in ((ra, da), (rb, db)):
            for key in ("iterations", "status", "trials_f", "trials_fg", "commits", "h_min", "h_max"):
                assert a[key] == b[key], key
            assert bits([a["f"]])[0] == bits([b["f"]])[0] and bits([a["gnorm"]])[0] == bits([b["gnorm"]])[0]
        assert np.array_equal(bits(host(xd)), bits(xh))
        assert np.array_equal(bits(host(c.get_x_device())), bits(xh))
        for key in ("tr_f", "tr_gnorm"):
            assert np.array_equal(bits(td[key]), bits(th[key])), key
        assert np.array_equal(bits(host(t0)), bits(x0))
        for big in (big0, bigx):
            assert host(big[0]) == SENTINEL and host(big[n + 1]) == SENTINEL


def test_host_objective_with_device_buffers():
    obj, n, m, ls, iters = "rosenbrock", 513, 3, "wolfe", 20
    x0 = O.x0_uniform(n, 42, -2.0, 2.0)
    la, lb = H.Log(obj), H.Log(obj)
    with L.Context(n, m) as c:
        ra = c.minimize("host", x0, ls, iters, f=la.f, grad=la.grad, trace=True)
        rb = c.minimize_device("host", dev(x0), ls, iters, f=lb.f, grad=lb.grad, trace=True)
    same_run(rb, ra)
    assert la.calls == lb.calls


# ---- 4. failure paths ----------------------------------------------------------------------------
def quad_fn(x, want_grad):
    e = x - 1.0
    f = float((e * e).sum())
    return (f, 2.0 * e) if want_grad else f


def refused(call, *a, **k):
    with pytest.raises(L.LbfgsError) as e:
        call(*a, **k)
    assert e.value.rc == BAD_ARG, e.value


def test_refusals():
    n, m = 513, 3
    x0 = O.x0_uniform(n, 42, -2.0, 2.0)
    t0 = dev(x0)
    calls = []

    def counted(x, want_grad):
        calls.append(want_grad)
        return quad_fn(x, want_grad)

    with L.Context(n, m) as c:
        refused(c.minimize_device, "device", t0, max_iterations=3)      # no objective set
        refused(c.minimize, "device", x0, max_iterations=3)
        refused(c.init_device, "device", t0)
        c.set_device_objective(counted)
        for flag in ("unfused", "vector_free", "reference_calls", "cuda_compat"):
            refused(c.minimize_device, "device", t0, max_iterations=3, **{flag: True})
            refused(c.minimize, "device", x0, max_iterations=3, **{flag: True})
        refused(c.line_search, "device", "backtracking", x0, -x0, x0)
        refused(c.objective, "device", x0)
        refused(c.trial, "device", x0, -x0, 0.5)
        assert not calls  # nothing reached the objective
        r = c.minimize_device("device", t0, max_iterations=3)
        assert calls and r["iterations"] >= 1
        c.set_device_objective(None)
        refused(c.minimize_device, "device", t0, max_iterations=3)


def test_refused_on_a_sharded_context():
    """world != 1: the objective cannot be set and the device-buffer forms are refused (nothing is
    launched, so the other rank is not needed)."""
    n, m = 4_000_003, 2
    grp = L.HostGroup(2)
    ctxs = [L.Context(n, m, rank=r, group=grp) for r in range(2)]
    try:
        t0 = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        refused(ctxs[0].set_device_objective, quad_fn)
        refused(ctxs[0].minimize_device, "device", t0, max_iterations=2)
        refused(ctxs[0].minimize_device, "rosenbrock", t0, max_iterations=2)
        refused(ctxs[0].init_device, "rosenbrock", t0)
        refused(ctxs[0].get_x_device, t0)
    finally:
        for c in ctxs:
            c.close()
        grp.close()


def test_callback_returning_nonzero_then_builtin():
    n, m, ls, iters = 513, 3, "backtracking", 10
    x0 = O.x0_uniform(n, 42, -2.0, 2.0)
    t0, tx = dev(x0), dev(np.zeros(n))
    with L.Context(n, m) as fresh:
        ref = fresh.minimize("rosenbrock", x0, ls, iters, trace=True)
    ncalls = [0]

    def ev(xp, nn, fp, gp, user):
        ncalls[0] += 1
        return 3

    cb = L.DEVICE_EVAL(ev)
    with L.Context(n, m) as c:
        fn = L.DeviceFn(cb, None, 0)
        assert L.lib().lbfgs_set_device_objective(c.h, C.byref(fn)) == 0
        k, res = L.constants(), L.Result()
        rc = L.lib().lbfgs_minimize_device(c.h, L.OBJECTIVES["device"], None, 0, C.byref(k), t0.data_ptr(),
                                           tx.data_ptr(), iters, 1e-5, L.FLAG_QUIET, C.byref(res))
        assert rc == ERR_CALLBACK and ncalls[0] == 1
        assert b"callback" in L.lib().lbfgs_last_error(c.h)
        same_run(c.minimize_device("rosenbrock", t0, ls, iters, trace=True), ref)


def test_python_exception_is_reraised():
    n, m = 513, 3
    x0 = O.x0_uniform(n, 42, -2.0, 2.0)
    calls = [0]

    class Boom(Exception):
        pass

    def fn(x, want_grad):
        calls[0] += 1
        if calls[0] == 3:
            raise Boom("third call")
        return quad_fn(x, want_grad)

    with L.Context(n, m) as c:
        c.set_device_objective(fn)
        with pytest.raises(Boom):
            c.minimize_device("device", dev(x0), max_iterations=10)
        assert calls[0] == 3
        c.set_device_objective(quad_fn)  # and the context goes on
        r = c.minimize_device("device", dev(x0), max_iterations=10)
        assert r["status"] == "converged"
        calls[0] = 0  # the stepping form: the third call is in step()
        c.set_device_objective(fn)
        c.init_device("device", dev(x0))
        with pytest.raises(Boom):
            c.step(10)


# ---- 5. the reducer --------------------------------------------------------------------------------
REDUCER_SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 1537, 65535, 65536, 65537, 2097152, 2097153, 5000000]


def between_nans(values, offset):
    """values at element `offset` of a NaN-filled allocation (offset 2: 16-byte aligned, 1: not)"""
    n = len(values)
    big = torch.full((n + 4,), float("nan"), dtype=torch.float64, device="cuda:0")
    t = big[offset:offset + n]
    t.copy_(dev(values))
    assert (t.data_ptr() % 16 == 0) == (offset == 2) and t.data_ptr() % 8 == 0
    return t


@pytest.mark.parametrize("n", REDUCER_SIZES)
def test_reducer_vs_oracle_and_context_dot(n):
    rng = np.random.default_rng(1000 + n % 997)
    a, b = rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n)
    want_dot = O.dot(a, b, O.CANON)
    want_sum = O.dot(a, np.ones(n), O.CANON)
    with L.Context(n, 1) as c:
        assert bits([c.dot(a, b)])[0] == bits([want_dot])[0]
    with L.Reducer(n) as red:
        for oa, ob in ((2, 2), (1, 1), (2, 1)):
            ta, tb = between_nans(a, oa), between_nans(b, ob)
            got = red.dot(ta, tb)
            assert bits([got])[0] == bits([want_dot])[0], (n, oa, ob, got, want_dot)
            got = red.sum(ta)
            assert bits([got])[0] == bits([want_sum])[0], (n, oa, got, want_sum)
        # the value does not depend on what ran before it
        assert bits([red.dot(ta, tb)])[0] == bits([want_dot])[0]


def test_reducer_rejects_other_tensors():
    with L.Reducer(100) as red:
        ok = torch.zeros(100, dtype=torch.float64, device="cuda:0")
        assert red.sum(ok) == 0.0
        for bad in (torch.zeros(99, dtype=torch.float64, device="cuda:0"),
                    torch.zeros(100, dtype=torch.float32, device="cuda:0"), torch.zeros(100, dtype=torch.float64),
                    torch.zeros(200, dtype=torch.float64, device="cuda:0")[::2]):
            with pytest.raises(ValueError):
                red.sum(bad)
            with pytest.raises(ValueError):
                red.dot(ok, bad)
