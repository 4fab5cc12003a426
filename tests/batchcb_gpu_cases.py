"""The GPU cases of tests/test_gpu_batch_callback.py, which runs this file in a process of its own
(torch is imported before the library is loaded, so that both use one HIP runtime).

The batched solver with a caller's objective for the whole batch (lbfgs_batch_set_device_objective,
Batch.set_device_objective): one call of fn(Z, active) -> (F, G) per round. Everything compares bits
(same_bits' NaN rule). The references are the canonical-order oracle with the same f / grad as host
callables, and the single-problem path, Context.set_device_objective(eager_grad=True) +
Context.minimize_device("device"), both computed once per case and shared.

1. against the single-problem path and the oracle: rosenbrock and quad_tridiag x the four searches,
   n = 1 (one element, no stencil neighbour), 5 (one partial row), 513 (a second segment of one
   element), 1537 (four segments), m = 1 and 5, B = 4, 30 iterations at most. The four x0 are
   O.x0_uniform at seeds 1..4: two in [-2, 2], one of those scaled by 1e-3, and one within 1e-4 of
   the all-ones point, Rosenbrock's minimiser, so that the problems end at different iterations.
   The tolerance is 1e-3 for Rosenbrock (at 1e-5 every start runs into the limit of 30) and 1e-5
   for the quadratic. test_inputs_exercise_the_paths asserts on the CPU, with the oracle alone, that
   every batch with n > 1 has every problem at 3 iterations or more, a search beyond its first trial
   and two different iteration counts. No seed can give that at n = 1: Rosenbrock has no term there
   (f = 0, 0 iterations) and the one-dimensional quadratic has its gradient at exactly 0 after 2
   iterations (with the tolerance at 1e-9 or 1e-13 one or two of the four starts take a third, the
   others still 2; at 0 all four run to the limit on a zero gradient); those cases stay, for the
   indexing, and the assertion says what they do reach;
2. rounds: as many calls as the largest f_calls, problem p active in exactly its first f_calls[p];
3. inactive rows are not read: NaN in F and G there, the same bits;
4. launch shape: 1 and 2 workgroups for 5 problems;
5. real device math: torch objectives per row, f through Reducer.sum, from minimize and from
   minimize_device on rows at storage offset 1, and on a non-default torch stream;
6. the guard inputs of tests/test_gpu_batch.py: event counts and statuses against the oracle's lines;
7. refusals, a failing callback, a Python exception, clearing, and the batch's other objectives;
8. a history of 16 pairs, the most a batch accepts, and of 8, filled and rotated (tests/hist_cases.py),
   which also runs the single-problem LBFGS_OBJ_DEVICE reference at m = 16;
9. the size limit, n = 32768;
10. line-search constants that are not the defaults (tests/consts_cases.py, path 12), and one row
    alone in a search of hundreds of rounds (backtracking_alpha = 0.99) beside two finished rows.
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
import hist_cases as HC  # noqa: E402
import lbfgs_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import test_gpu_batch as S  # noqa: E402  (same_bits, check_problem, message_counts, GUARD_BATCHES)
import test_gpu_host_callbacks as H  # noqa: E402  (Log: the oracle's f / grad as callables)
import devobj_gpu_cases as DV  # noqa: E402  (DeviceLog, torch_rosenbrock, torch_separable)

pytestmark = pytest.mark.gpu

BAD_ARG, ERR_CALLBACK = -1, -6
DEV = "cuda:0"
same_bits = S.same_bits
SEARCHES = S.SEARCHES
OBJS1 = ["rosenbrock", "quad_tridiag"]
SIZES1 = [1, 5, 513, 1537]
MS1 = [1, 5]
MAXIT1 = 30
TOL1 = {"rosenbrock": 1e-3, "quad_tridiag": 1e-5}
COUNTS = ("iterations", "trials_f", "trials_fg", "commits", "h_min", "h_max")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


def host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


x0_batch = HC.x0_batch  # (the four starts; the CPU condition tests need them without torch)


class BatchLog:
    """fn(Z, active) that brings each active row to the CPU and calls the oracle's f / grad (H.Log's
    callables, as DeviceLog does for one problem). `fill` is what F and G hold for inactive rows."""

    def __init__(self, obj, fill=0.0):
        self.log, self.fill = H.Log(obj), fill
        self.rounds = []  # the active view of every call

    def __call__(self, Z, active):
        act = active.cpu().numpy().copy()
        self.rounds.append(act)
        B, n = Z.shape
        F, G = np.full(B, self.fill), np.full((B, n), self.fill)
        for p in np.flatnonzero(act):
            xh = host(Z[p])
            F[p] = self.log.f(xh)
            G[p] = self.log.grad(xh)
        return dev(F), dev(G)


_reference = {}


def device_constants(consts):
    """lbfgs_constants with the fields of a dictionary replaced (None: the defaults)"""
    k = L.constants()
    for name, v in (consts or {}).items():
        setattr(k, name, v)
    return k


def reference(obj, ls, n, m, X0, maxit, tol, key, consts=None):
    """(oracle runs, single-problem runs) of a batch, computed once per key and shared (left unchanged).
    consts: a dictionary of line-search constants that replace the defaults in both."""
    if key not in _reference:
        orc, one = [], []
        with L.Context(n, m) as c:
            for x0 in X0:
                lo = H.Log(obj)
                with np.errstate(all="ignore"):
                    orc.append(O.lbfgs("host", x0, ls, m, maxit, tol, mode=O.CANON, f=lo.f, grad=lo.grad, consts=consts))
                c.set_device_objective(DV.DeviceLog(obj), eager_grad=True)
                r = c.minimize_device("device", dev(x0), ls, maxit, tol, trace=True, consts=device_constants(consts))
                r["x"] = host(r["x"])
                one.append(r)
        _reference[key] = (orc, one)
    return _reference[key]


def check_single(res, p, one, what):
    """problem p of a batch result against the single-problem path's run of it"""
    assert same_bits(host(res["x"][p]), one["x"]), (what, p)
    assert same_bits([res["f"][p], res["gnorm"][p]], [one["f"], one["gnorm"]]), (what, p)
    assert res["status"][p] == one["status"], (what, p, res["status"][p], one["status"])
    for key in COUNTS:
        assert res[key][p] == one[key], (what, p, key, res[key][p], one[key])
    assert same_bits(res["tr_f"][p], one["tr_f"]) and same_bits(res["tr_gnorm"][p], one["tr_gnorm"]), (what, p)
    assert same_bits(res["tr_alpha"][p], one["tr_alpha"]), (what, p)
    want = S.message_counts(one)
    assert [res["events"][p][k] for k in S.EVENT_KEYS] == want[:4], (what, p)
    assert res["f_calls"][p] == res["grad_calls"][p], (what, p)
    if np.all(np.isfinite(one["tr_f"])):
        assert res["f_calls"][p] == one["grad_calls"], (what, p, res["f_calls"][p], one["grad_calls"])


def check_batch(res, orc, one, what):
    for p in range(len(orc)):
        S.check_problem(dict(res, x=[host(x) for x in res["x"]]), p, orc[p], what)
        check_single(res, p, one[p], what)


def case1(obj, ls, n, m):
    X0 = x0_batch(n)
    return X0, reference(obj, ls, n, m, X0, MAXIT1, TOL1[obj], ("case1", obj, ls, n, m))


# ---- 1. against the single-problem path and the oracle ------------------------------------------
def test_inputs_exercise_the_paths():
    """On the CPU, with the oracle alone (the module docstring says what n = 1 cannot give)."""
    for obj in OBJS1:
        for ls in SEARCHES:
            for n in SIZES1:
                for m in MS1:
                    its, beyond, first = [], [], L.constants().initial_step
                    for x0 in x0_batch(n):
                        lo = H.Log(obj)
                        o = O.lbfgs("host", x0, ls, m, MAXIT1, TOL1[obj], mode=O.CANON, f=lo.f, grad=lo.grad)
                        a = o["alpha"][np.isfinite(o["alpha"])]
                        its.append(o["iters"])
                        beyond.append(bool(np.any(a != first)))  # an accepted step that is not the first trial's
                    what = (obj, ls, n, m, its)
                    if n > 1:
                        assert min(its) >= 3 and any(beyond) and len(set(its)) >= 2, what
                    elif obj == "rosenbrock":
                        assert its == [0, 0, 0, 0], what
                    else:
                        assert min(its) >= 1 and any(beyond), what


@pytest.mark.parametrize("m", MS1)
@pytest.mark.parametrize("n", SIZES1)
@pytest.mark.parametrize("ls", SEARCHES)
@pytest.mark.parametrize("obj", OBJS1)
def test_batch_callback_vs_single_path_and_oracle(obj, ls, n, m):
    X0, (orc, one) = case1(obj, ls, n, m)
    fn = BatchLog(obj)
    with L.Batch(n, m, len(X0)) as b:
        b.set_device_objective(fn)
        res = b.minimize("device", X0, ls, max_iterations=MAXIT1, tolerance=TOL1[obj], trace=True)
    check_batch(res, orc, one, (obj, ls, n, m))
    assert res["launches"] == len(fn.rounds) + 1


# ---- 2. rounds -------------------------------------------------------------------------------------
def check_rounds(fn, res):
    calls = np.array(res["f_calls"])
    assert len(fn.rounds) == calls.max(), (len(fn.rounds), calls)
    for p, k in enumerate(calls):
        got = [bool(r[p]) for r in fn.rounds]
        assert got == [True] * int(k) + [False] * (len(fn.rounds) - int(k)), (p, k, got)


@pytest.mark.parametrize("obj,ls,n,m", [("quad_tridiag", "wolfe", 513, 5), ("rosenbrock", "backtracking", 1537, 1)])
def test_rounds(obj, ls, n, m):
    X0, (orc, one) = case1(obj, ls, n, m)
    fn = BatchLog(obj)
    with L.Batch(n, m, len(X0)) as b:
        b.set_device_objective(fn)
        res = b.minimize("device", X0, ls, max_iterations=MAXIT1, tolerance=TOL1[obj], trace=True)
    check_rounds(fn, res)
    assert len(set(res["f_calls"])) >= 2
    assert [int(r.sum()) for r in fn.rounds] == [int(np.sum(np.array(res["f_calls"]) > i)) for i in range(len(fn.rounds))]


def test_a_problem_at_the_minimiser_is_active_once():
    n, m = 513, 3
    X0 = np.stack([O.x0_uniform(n, 1, -2.0, 2.0), np.ones(n), O.x0_uniform(n, 2, -2.0, 2.0)])
    fn = BatchLog("quad_sep")
    with L.Batch(n, m, 3) as b:
        b.set_device_objective(fn)
        res = b.minimize("device", X0, "backtracking", max_iterations=10, trace=True)
    check_rounds(fn, res)
    assert res["f_calls"][1] == 1 and res["iterations"][1] == 0 and res["status"][1] == "converged"
    assert [bool(r[1]) for r in fn.rounds] == [True] + [False] * (len(fn.rounds) - 1)
    assert same_bits(res["x"][1], np.ones(n)) and res["iterations"][0] >= 1


# ---- 3. inactive rows are not read -----------------------------------------------------------------
@pytest.mark.parametrize("obj,ls,n,m", [("rosenbrock", "wolfe", 513, 5), ("quad_tridiag", "backtracking", 1537, 1),
                                        ("quad_tridiag", "backtracking_wolfe", 5, 5)])
def test_inactive_rows_are_not_read(obj, ls, n, m):
    X0, (orc, one) = case1(obj, ls, n, m)
    fn = BatchLog(obj, fill=float("nan"))
    with L.Batch(n, m, len(X0)) as b:
        b.set_device_objective(fn)
        res = b.minimize("device", X0, ls, max_iterations=MAXIT1, tolerance=TOL1[obj], trace=True)
    assert any(not r.all() for r in fn.rounds)  # some round had an inactive row
    check_batch(res, orc, one, ("nan fill", obj, ls, n, m))


# ---- 4. launch shape --------------------------------------------------------------------------------
def test_launch_shape_does_not_matter():
    obj, ls, n, m, B, maxit = "quad_tridiag", "wolfe", 513, 3, 5, 12
    X0 = S.seeds_x0(n, range(1, B + 1), -2.0, 2.0)
    X0[1] *= 1e-3
    runs = []
    with L.Batch(n, m, B) as b:
        b.set_device_objective(BatchLog(obj))
        for wg in (0, 1, 2):
            b.set_launch(max_workgroups=wg)
            runs.append(b.minimize("device", X0, ls, max_iterations=maxit, trace=True))
    base = runs[0]
    assert len(set(base["iterations"])) >= 2 and min(base["iterations"]) >= 3
    for r in runs[1:]:
        assert same_bits(r["x"], base["x"]) and same_bits(r["f"], base["f"]) and same_bits(r["gnorm"], base["gnorm"])
        for key in COUNTS + ("f_calls", "grad_calls", "status_code"):
            assert list(r[key]) == list(base[key]), key
        for p in range(B):
            for key in ("tr_f", "tr_gnorm", "tr_alpha"):
                assert same_bits(r[key][p], base[key][p]), (key, p)
            assert r["events"][p] == base["events"][p]


# ---- 5. real device math ----------------------------------------------------------------------------
def per_row(single):
    """fn(Z, active) from a single-problem fn(x, want_grad): the active rows, one after another"""
    def fn(Z, active):
        B, n = Z.shape
        F = torch.full((B,), float("nan"), dtype=torch.float64, device=Z.device)
        G = torch.full((B, n), float("nan"), dtype=torch.float64, device=Z.device)
        for p in np.flatnonzero(active.cpu().numpy()):
            f, g = single(Z[p], True)
            F[p] = f
            G[p] = g
        return F, G

    return fn


@pytest.mark.parametrize("make", [DV.torch_rosenbrock, DV.torch_separable])
@pytest.mark.parametrize("ls", ["wolfe", "backtracking"])
def test_torch_objective_batch_vs_single(make, ls):
    n, m, B, iters = 2000, 5, 3, 30
    X0 = S.seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    X0[1] *= 1e-3
    side = torch.cuda.Stream(device=DEV)
    with L.Reducer(n) as red, L.Context(n, m) as c, L.Batch(n, m, B) as b:
        single = make(red)
        c.set_device_objective(single, eager_grad=True)
        one = []
        for x0 in X0:
            r = c.minimize_device("device", dev(x0), ls, iters, trace=True)
            r["x"] = host(r["x"])
            one.append(r)
        assert max(r["iterations"] for r in one) >= 2  # (the separable quadratic needs no more under backtracking)
        fn = per_row(single)

        def on_side(Z, active):
            with torch.cuda.stream(side):  # the reducer runs on the current stream: this one
                assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
                r = fn(Z, active)
            side.synchronize()  # F and G are complete before the glue copies them
            return r

        # rows at storage offset 1 of NaN-filled (x0) and sentinel-filled (x) allocations, stride n + 3
        ld = n + 3
        buf0 = torch.full((1 + B * ld,), float("nan"), dtype=torch.float64, device=DEV)
        bufx = torch.full((1 + B * ld,), DV.SENTINEL, dtype=torch.float64, device=DEV)
        T0, TX = buf0.as_strided((B, n), (ld, 1), 1), bufx.as_strided((B, n), (ld, 1), 1)
        T0.copy_(dev(X0))
        for f, form in ((fn, "host"), (fn, "device"), (on_side, "host")):
            b.set_device_objective(f)
            if form == "host":
                res = b.minimize("device", X0, ls, max_iterations=iters, trace=True)
            else:
                res = b.minimize_device("device", T0, ls, max_iterations=iters, trace=True, out=TX)
                assert res["x"] is TX
                outside = np.ones(1 + B * ld, bool)
                for p in range(B):
                    outside[1 + p * ld:1 + p * ld + n] = False
                assert np.all(host(bufx)[outside] == DV.SENTINEL) and same_bits(host(T0), X0)
            for p in range(B):
                check_single(res, p, one[p], (make.__name__, ls, form, f is on_side))
                # at a step that is not a number the single path evaluates the same point twice, the batch once
                if not np.all(np.isfinite(one[p]["tr_alpha"][:-1])):
                    assert 0 < res["f_calls"][p] <= one[p]["grad_calls"], (p, res["f_calls"][p], one[p]["grad_calls"])
        if make is DV.torch_separable and ls == "wolfe":  # the case that reaches such steps
            assert any(not np.all(np.isfinite(r["tr_f"])) for r in one)


# ---- 6. guard paths ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.GUARD_BATCHES, ids=lambda c: f"{c[0]}-{c[1]}-n{c[2]}-m{c[3]}")
def test_guard_paths(case):
    obj, ls, n, m, lo, hi, maxit, tol = case
    X0 = S.seeds_x0(n, [1, 2, 3], lo, hi)
    orc, one = reference(obj, ls, n, m, X0, maxit, tol, ("guard",) + case)
    with L.Batch(n, m, 3) as b:
        b.set_device_objective(BatchLog(obj))
        res = b.minimize("device", X0, ls, max_iterations=maxit, tolerance=tol, trace=True)
    check_batch(res, orc, one, case)
    for p in range(3):
        want = S.message_counts(orc[p])
        assert [res["events"][p][k] for k in S.EVENT_KEYS] == want[:4], (case, p, want)
        assert (res["status"][p] == "ls_failed") == (want[4] > 0), (case, p)


def test_guard_inputs_reach_the_guards():
    """On the CPU: the not-descent fallback, a skipped update and a failed line search each occur
    somewhere in these batches, with the objective as callables too."""
    total = np.zeros(len(S.MESSAGES), dtype=int)
    for case in S.GUARD_BATCHES:
        obj, ls, n, m, lo, hi, maxit, tol = case
        for x0 in S.seeds_x0(n, [1, 2, 3], lo, hi):
            lg = H.Log(obj)
            total += np.array(S.message_counts(O.lbfgs("host", x0, ls, m, maxit, tol, mode=O.CANON, f=lg.f, grad=lg.grad)))
    assert total[0] > 0 and total[1] > 0 and total[4] > 0, dict(zip(S.MESSAGES, total))


# ---- 7. refusals and errors ---------------------------------------------------------------------------
def refused(call, *a, **k):
    with pytest.raises(L.LbfgsError) as e:
        call(*a, **k)
    assert e.value.rc == BAD_ARG, e.value
    return str(e.value)


def test_device_with_nothing_set_is_refused():
    n, m, B = 5, 2, 3
    X0 = S.seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    with L.Batch(n, m, B) as b:
        refused(b.minimize, "device", X0, max_iterations=3)
        refused(b.minimize_device, "device", dev(X0), max_iterations=3)


def test_refusals_and_clearing():
    n, m, B = 5, 2, 3
    X0 = S.seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    fn = BatchLog("quad_sep")
    with L.Batch([5, 3, 4], m) as rag:
        assert "ragged" in refused(rag.set_device_objective, fn)
        refused(rag.minimize, "device", [X0[0], X0[1][:3], X0[2][:4]], max_iterations=3)
    with L.Batch(n, m, B) as b:
        null = L.BatchDeviceFn(L.BATCH_DEVICE_EVAL(), None, 0)
        assert L.lib().lbfgs_batch_set_device_objective(b.h, C.byref(null)) == BAD_ARG
        refused(b.minimize, "device", X0, max_iterations=3)
        b.set_device_objective(fn)
        for flag in (L.FLAG_VERBOSE, L.FLAG_UNFUSED, L.FLAG_VECTOR_FREE, L.FLAG_REFERENCE_CALLS):
            refused(b.minimize, "device", X0, max_iterations=3, flags=flag)
        assert not fn.rounds  # nothing reached the objective
        r = b.minimize("device", X0, max_iterations=3)
        assert fn.rounds and min(r["iterations"]) >= 1
        b.set_device_objective(None)
        refused(b.minimize, "device", X0, max_iterations=3)
        refused(b.minimize_device, "device", dev(X0), max_iterations=3)
        assert L.lib().lbfgs_batch_set_device_objective(None, None) == BAD_ARG


def test_callback_returning_nonzero_then_the_batch_goes_on():
    obj, ls, n, m, B, iters = "rosenbrock", "backtracking", 513, 3, 3, 10
    X0 = S.seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    orc, one = reference(obj, ls, n, m, X0, iters, 1e-5, ("nonzero",))
    ncalls = [0]

    def ev(zp, ldz, fp, gp, ldg, ap, n_active, batch, nn, user):
        ncalls[0] += 1
        assert n_active == B and batch == B and nn == n and ldz > n and ldg > n
        return 3

    cb = L.BATCH_DEVICE_EVAL(ev)
    with L.Batch(n, m, B) as b:
        fresh = b.minimize(obj, X0, ls, max_iterations=iters, trace=True)
        fnc = L.BatchDeviceFn(cb, None, 0)
        assert L.lib().lbfgs_batch_set_device_objective(b.h, C.byref(fnc)) == 0
        k, res, X = L.constants(), (L.Result * B)(), np.zeros_like(X0)
        rc = L.lib().lbfgs_batch_minimize(b.h, L.OBJECTIVES["device"], L.LINE_SEARCHES[ls], C.byref(k), X0, X, iters,
                                          1e-5, L.FLAG_QUIET, res)
        assert rc == ERR_CALLBACK and ncalls[0] == 1
        assert b"callback" in L.lib().lbfgs_batch_last_error(b.h)
        again = b.minimize(obj, X0, ls, max_iterations=iters, trace=True)
        assert same_bits(again["x"], fresh["x"]) and same_bits(again["f"], fresh["f"])
        assert list(again["iterations"]) == list(fresh["iterations"])
        b.set_device_objective(BatchLog(obj))
        check_batch(b.minimize("device", X0, ls, max_iterations=iters, trace=True), orc, one, "after a nonzero return")


def test_python_exception_is_reraised():
    n, m, B = 513, 3, 3
    X0 = S.seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    good = BatchLog("quad_sep")
    calls = [0]

    class Boom(Exception):
        pass

    def fn(Z, active):
        calls[0] += 1
        if calls[0] == 3:
            raise Boom("third round")
        return good(Z, active)

    with L.Batch(n, m, B) as b:
        b.set_device_objective(fn)
        with pytest.raises(Boom):
            b.minimize("device", X0, max_iterations=10)
        assert calls[0] == 3
        with pytest.raises(Boom):
            calls[0] = 2
            b.minimize_device("device", dev(X0), max_iterations=10)
        b.set_device_objective(good)  # and the batch goes on
        r = b.minimize("device", X0, max_iterations=10)
        assert r["status"] == ["converged"] * B


def test_other_objectives_of_the_batch_are_undisturbed():
    n, m, B, iters = 65, 3, 3, 8
    X0 = S.seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    rng = np.random.default_rng(7)
    Q = rng.uniform(-1.0, 1.0, (B, n, n))
    A = np.einsum("bij,bkj->bik", Q, Q) / n + np.eye(n)
    bb = rng.uniform(-1.0, 1.0, (B, n))
    keys = ("x", "f", "gnorm", "iterations", "status_code", "trials_f", "trials_fg", "commits", "bytes")

    def same(r, s, what):
        for key in keys:
            assert same_bits(r[key], s[key]), (what, key)
        for p in range(B):
            assert same_bits(r["tr_f"][p], s["tr_f"][p]) and r["events"][p] == s["events"][p], (what, p)

    with L.Batch(n, m, B) as b:
        b.set_dense_quadratics(A, bb)
        st0 = b.minimize("rosenbrock", X0, "wolfe", max_iterations=iters, trace=True)
        dq0 = b.minimize("dense", X0, "wolfe", max_iterations=iters, trace=True)
        b.set_device_objective(BatchLog("quad_tridiag"))
        dv0 = b.minimize("device", X0, "wolfe", max_iterations=iters, trace=True)
        assert min(dv0["iterations"]) >= 3 and min(dv0["f_calls"]) > 0
        same(b.minimize("rosenbrock", X0, "wolfe", max_iterations=iters, trace=True), st0, "stencil")
        same(b.minimize("dense", X0, "wolfe", max_iterations=iters, trace=True), dq0, "dense")
        assert list(st0["f_calls"]) == [0] * B and list(dq0["f_calls"]) == [0] * B
        same(b.minimize("device", X0, "wolfe", max_iterations=iters, trace=True), dv0, "device again")
        b.set_device_objective(None)
        same(b.minimize("dense", X0, "wolfe", max_iterations=iters, trace=True), dq0, "dense after clearing")


# ---- 8. a history of 16 pairs, and of 8 (tests/hist_cases.py) -----------------------------------------
@pytest.mark.parametrize("case", HC.STENCIL, ids=HC.case_id)
def test_long_history(case):
    """m = 16, the largest history a batch accepts, and m = 8, on inputs that fill the ring and rotate it
    (tests/test_history_inputs.py asserts that on the CPU, with the objective as callables): the oracle,
    and the single-problem LBFGS_OBJ_DEVICE path at the same m."""
    obj, n, m, ls, tol, differ = case
    X0 = HC.stencil_x0(case)
    orc, one = reference(obj, ls, n, m, X0, HC.MAXIT, tol, ("hist",) + case)
    fn = BatchLog(obj)
    with L.Batch(n, m, len(X0)) as b:
        b.set_device_objective(fn)
        res = b.minimize("device", X0, ls, max_iterations=HC.MAXIT, tolerance=tol, trace=True)
    check_batch(res, orc, one, case)
    check_rounds(fn, res)
    HC.check_h_max(res, orc, m, case)
    assert all(one[p]["h_max"] == m for p in range(len(X0)) if HC.full_ring(orc[p], m))
    assert not differ or len(set(res["iterations"])) >= 2


# ---- 9. the size limit ---------------------------------------------------------------------------------
def test_size_limit():
    """n = 32768, the largest a batch accepts: 64 segments, every lane of the stage-2 wave live"""
    obj, ls, n, m, maxit = "rosenbrock", "backtracking", 32768, 3, 6
    assert O.geometry(n) == (512, 64)
    X0 = S.seeds_x0(n, [1, 2], -2.0, 2.0)
    orc, one = reference(obj, ls, n, m, X0, maxit, 1e-5, ("limit",))
    assert all(o["iters"] == maxit for o in orc)
    fn = BatchLog(obj)
    with L.Batch(n, m, len(X0)) as b:
        b.set_device_objective(fn)
        res = b.minimize("device", X0, ls, max_iterations=maxit, tolerance=1e-5, trace=True)
    check_batch(res, orc, one, "n=32768")
    check_rounds(fn, res)
    assert list(res["h_max"]) == [m, m]


# ---- 10. line-search constants that are not the defaults (tests/consts_cases.py, path 12) -------------
@pytest.mark.parametrize("case", K.BATCH_CALLBACK, ids=lambda c: "-".join(str(v) for v in c))
def test_varied_constants(case):
    """A search here is an lbk_search record stored between launches and resumed: constants that are no
    powers of two tell a stored step from a recomputed one. tests/test_constants_inputs.py asserts on the
    CPU that the constants bite in every batch and what each reaches (failed searches beside problems
    that run on, Wolfe expanding every iteration, backtracking-Wolfe growing a step some 24 times in every search)."""
    ks, obj, n, m, ls, iters = case
    X0 = K.batch_x0(n)
    orc, one = reference(obj, ls, n, m, X0, iters, K.TOL, ("consts",) + case, consts=K.SETS[ks])
    fn = BatchLog(obj)
    with L.Batch(n, m, len(X0)) as b:
        b.set_device_objective(fn)
        res = b.minimize("device", X0, ls, max_iterations=iters, tolerance=K.TOL, consts=device_constants(K.SETS[ks]),
                         trace=True)
    print(f"{case}: {len(fn.rounds)} rounds, f_calls {list(res['f_calls'])}")
    check_batch(res, orc, one, case)
    check_rounds(fn, res)
    assert res["launches"] == len(fn.rounds) + 1


def test_one_row_alone_in_a_long_search():
    """backtracking_alpha = 0.99: the middle row's first search rejects hundreds of steps, a round each,
    while the rows beside it, done after their first evaluation, stay inactive: the record alone carries
    the search from launch to launch. Its step and x against the single-problem path and the oracle."""
    c = K.LONG_SEARCH
    obj, ls, n, m, iters, row = c["objective"], c["search"], c["n"], c["m"], c["iterations"], c["row"]
    X0 = K.long_search_x0()
    orc, one = reference(obj, ls, n, m, X0, iters, K.TOL, ("long search",), consts=c["consts"])
    fn = BatchLog(obj)
    with L.Batch(n, m, len(X0)) as b:
        b.set_device_objective(fn)
        res = b.minimize("device", X0, ls, max_iterations=iters, tolerance=K.TOL, consts=device_constants(c["consts"]),
                         trace=True)
    print(f"long search: {len(fn.rounds)} rounds, f_calls {list(res['f_calls'])}")
    check_batch(res, orc, one, "long search")
    check_rounds(fn, res)
    others = [p for p in range(len(X0)) if p != row]
    step = res["tr_alpha"][row][0]
    assert same_bits([step], [orc[row]["alpha"][0]]) and same_bits([step], [one[row]["tr_alpha"][0]])
    assert same_bits(host(res["x"][row]), orc[row]["x"]) and same_bits(host(res["x"][row]), one[row]["x"])
    assert all(res["f_calls"][p] == 1 and res["iterations"][p] == 0 and res["status"][p] == "converged" for p in others)
    alone = fn.rounds[1:]
    assert len(alone) >= c["rejected_at_least"] and res["f_calls"][row] == len(fn.rounds)
    assert all(r[row] and not any(r[p] for p in others) for r in alone)
