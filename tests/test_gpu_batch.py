"""GPU tests of the batched small-n solver (lbfgs_batch_*, L.Batch): B problems, one workgroup each,
the whole solver loop on the device. Everything is compared bit for bit (never a tolerance): the
feature reorders launches, not arithmetic. The reference is the canonical-order oracle, run once
per problem on the CPU, and for two batches the single-problem path (Context.minimize).

Shapes are the smallest at which each mechanism can go wrong: n = 5 (one partial row, both stencil
edges in one wave), 512 (exactly one full segment), 513 (a second segment of one element: the seam
halo meets a 1-element segment), 1537 (four segments, the last of one element), 32768 (64
segments: every lane of the stage-2 wave live); m = 1 (a two-loop with no q pass), m = 5 with 12
iterations (the ring and the spare pair rotate), m = 16 and 8 with 40 iterations at most (the largest
history the batch accepts, filled and rotated; tests/hist_cases.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import hist_cases as HC  # noqa: E402
import lbfgs_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402

pytestmark = pytest.mark.gpu

OBJS = ["rosenbrock", "quad_tridiag", "quad_sep"]
SEARCHES = ["backtracking", "interpolation", "wolfe", "backtracking_wolfe"]
MESSAGES = ["Not a descent direction", "Skipping update", "Invalid rho", "Invalid gamma", "Line search failed"]
EVENT_KEYS = ["not_descent", "skipped_updates", "invalid_rho", "invalid_gamma"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def seeds_x0(n, seeds, lo, hi):
    return np.stack([O.x0_uniform(n, s, lo, hi) for s in seeds])


_oracle = {}


def oracle(obj, X0, ls, m, maxit, tol, key):
    """The oracle's runs of a batch, computed once per key and shared (left unchanged)."""
    if key not in _oracle:
        _oracle[key] = [O.lbfgs(obj, x0, ls, m, maxit, tol, mode=O.CANON) for x0 in X0]
    return _oracle[key]


def same_bits(a, b):
    """Equal bit for bit; a NaN equals a NaN in the same place (the separable quadratic under the
    Wolfe search diverges to NaN in the reference too, and a NaN's sign and payload are the
    processor's: x86 and the GPU produce different ones from the same operation)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def check_problem(res, p, o, what=""):
    """x, f, |g|, iterations, status and the traces of problem p against its oracle run. (The oracle
    records f at the top of every iteration and at the exit; after a failed line search the result's
    f is f at the failed step, which the oracle does not return: that one is compared with the
    single-problem path where a batch has such a problem.)"""
    assert res["status"][p] == o["status"], (what, p, res["status"][p], o["status"])
    assert res["iterations"][p] == o["iters"], (what, p)
    assert same_bits(res["x"][p], o["x"]), (what, p)
    assert same_bits([res["gnorm"][p]], [o["gnorm"][-1]]), (what, p)
    if o["status"] != "ls_failed":
        assert same_bits([res["f"][p]], [o["f"][-1]]), (what, p)
    assert len(res["tr_f"][p]) == len(o["f"]), (what, p)
    assert same_bits(res["tr_f"][p], o["f"]), (what, p)
    assert same_bits(res["tr_gnorm"][p], o["gnorm"]), (what, p)
    a1, a2 = res["tr_alpha"][p], o["alpha"]
    assert np.array_equal(np.isnan(a1), np.isnan(a2)), (what, p)
    assert same_bits(a1[~np.isnan(a1)], a2[~np.isnan(a2)]), (what, p)


def message_counts(o):
    return [sum(1 for line in o["messages"].splitlines() if m in line) for m in MESSAGES]


# ---- 1. parity matrix -------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("n", [5, 512, 513, 1537])
@pytest.mark.parametrize("ls", SEARCHES)
@pytest.mark.parametrize("obj", OBJS)
def test_parity_matrix(obj, ls, n, m):
    X0 = seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    orc = oracle(obj, X0, ls, m, 12, 1e-5, ("matrix", obj, ls, n, m))
    with L.Batch(n, m, 3) as b:
        res = b.minimize(obj, X0, ls, max_iterations=12, tolerance=1e-5, trace=True)
    for p in range(3):
        check_problem(res, p, orc[p], (obj, ls, n, m))


def test_parity_64_segments():
    n, m = 32768, 3
    assert O.geometry(n) == (512, 64)
    X0 = seeds_x0(n, [1, 2], -2.0, 2.0)
    orc = oracle("rosenbrock", X0, "backtracking", m, 6, 1e-5, ("seg64",))
    with L.Batch(n, m, 2) as b:
        res = b.minimize("rosenbrock", X0, "backtracking", max_iterations=6, tolerance=1e-5, trace=True)
    for p in range(2):
        check_problem(res, p, orc[p], "n=32768")


# ---- 2. problems of one batch end at different times ---------------------------------------------
def _mixed_batch():
    n = 513
    X0 = np.stack([O.x0_uniform(n, 1, -2.0, 2.0), O.x0_uniform(n, 2, -1e-3, 1e-3), O.x0_uniform(n, 3, -30.0, 30.0),
                   np.ones(n), np.zeros(n), 1.0 + O.x0_uniform(n, 4, -1e-4, 1e-4)])
    return n, 3, X0, oracle("quad_tridiag", X0, "wolfe", 3, 25, 1e-5, ("mixed",))


def test_problems_end_at_different_times():
    n, m, X0, orc = _mixed_batch()
    iters = [o["iters"] for o in orc]
    assert 0 in iters and len(set(iters)) >= 3, iters  # a condition on the inputs (CPU)
    with L.Batch(n, m, len(X0)) as b:
        res = b.minimize("quad_tridiag", X0, "wolfe", max_iterations=25, tolerance=1e-5, trace=True)
    for p in range(len(X0)):
        check_problem(res, p, orc[p], "mixed")
    assert list(res["iterations"]) == iters


# ---- 3. guard paths ----------------------------------------------------------------------------
GUARD_BATCHES = [  # (objective, line search, n, m, lo, hi, max_iterations, tol)
    ("rosenbrock", "wolfe", 5, 5, -1e-3, 1e-3, 60, 0.0),
    ("rosenbrock", "backtracking", 5, 5, -1e-3, 1e-3, 60, 0.0),
    ("rosenbrock", "backtracking_wolfe", 5, 5, -1e-3, 1e-3, 60, 0.0),
    ("quad_sep", "backtracking", 5, 1, -1e-3, 1e-3, 60, 0.0),
    ("quad_sep", "interpolation", 5, 1, -1e-3, 1e-3, 60, 0.0),
    ("rosenbrock", "backtracking", 1000, 5, -2.0, 2.0, 40, 1e-5),
]


def _guard_oracle(case):
    obj, ls, n, m, lo, hi, maxit, tol = case
    X0 = seeds_x0(n, [1, 2, 3], lo, hi)
    return X0, oracle(obj, X0, ls, m, maxit, tol, ("guard",) + case)


def test_guard_inputs_reach_the_guards():
    """A condition on the inputs, on the CPU: the not-descent fallback, a skipped update and a failed
    line search each occur somewhere in these batches."""
    total = np.zeros(len(MESSAGES), dtype=int)
    for case in GUARD_BATCHES:
        _, orc = _guard_oracle(case)
        for o in orc:
            total += np.array(message_counts(o))
    assert total[0] > 0 and total[1] > 0 and total[4] > 0, dict(zip(MESSAGES, total))


@pytest.mark.parametrize("case", GUARD_BATCHES, ids=lambda c: f"{c[0]}-{c[1]}-n{c[2]}-m{c[3]}")
def test_guard_paths(case):
    obj, ls, n, m, lo, hi, maxit, tol = case
    X0, orc = _guard_oracle(case)
    with L.Batch(n, m, 3) as b:
        res = b.minimize(obj, X0, ls, max_iterations=maxit, tolerance=tol, trace=True)
    for p in range(3):
        check_problem(res, p, orc[p], case)
        want = message_counts(orc[p])
        got = [res["events"][p][k] for k in EVENT_KEYS]
        assert got == want[:4], (case, p, got, want)
        assert (res["status"][p] == "ls_failed") == (want[4] > 0), (case, p)
        assert want[4] <= 1
        if res["status"][p] == "ls_failed":  # f at the failed step: the single-problem path's
            with L.Context(n, m) as c:
                one = c.minimize(obj, X0[p], ls, max_iterations=maxit, tolerance=tol)
            assert one["status"] == "ls_failed"
            assert same_bits([res["f"][p]], [one["f"]]), (case, p)


# ---- 4. launch shape does not matter -------------------------------------------------------------
def test_launch_shape_does_not_matter():
    n, m, B = 513, 3, 7
    X0 = seeds_x0(n, range(1, B + 1), -2.0, 2.0)
    orc = oracle("rosenbrock", X0, "interpolation", m, 10, 1e-5, ("shape",))
    with L.Batch(n, m, B) as b:
        for wg in (1, 2, 0):
            for ipl in (1, 3, 0):
                b.set_launch(max_workgroups=wg, iters_per_launch=ipl)
                res = b.minimize("rosenbrock", X0, "interpolation", max_iterations=10, tolerance=1e-5, trace=True)
                for p in range(B):
                    check_problem(res, p, orc[p], ("shape", wg, ipl))


# ---- 5. more problems than the card holds at once ------------------------------------------------
def test_more_problems_than_resident_workgroups():
    n, m, B = 5, 2, 3000
    X0 = seeds_x0(n, range(1, B + 1), -2.0, 2.0)
    with L.Batch(n, m, B) as b:
        res = b.minimize("quad_sep", X0, "backtracking", max_iterations=4, tolerance=1e-5, trace=True)
    for p in range(B):
        o = O.lbfgs("quad_sep", X0[p], "backtracking", m, 4, 1e-5, mode=O.CANON)
        check_problem(res, p, o, "B=3000")


# ---- 6. the same as the single-problem path ------------------------------------------------------
def _same_as_single(obj, ls, n, m, X0, maxit, tol):
    with L.Batch(n, m, len(X0)) as b:
        res = b.minimize(obj, X0, ls, max_iterations=maxit, tolerance=tol)
    with L.Context(n, m) as c:
        for p in range(len(X0)):
            one = c.minimize(obj, X0[p], ls, max_iterations=maxit, tolerance=tol)
            assert same_bits(res["x"][p], one["x"]), p
            assert same_bits([res["f"][p], res["gnorm"][p]], [one["f"], one["gnorm"]]), p
            assert res["iterations"][p] == one["iterations"] and res["status"][p] == one["status"], p


def test_same_as_single_problem_path_mixed():
    n, m, X0, _ = _mixed_batch()
    _same_as_single("quad_tridiag", "wolfe", n, m, X0, 25, 1e-5)


def test_same_as_single_problem_path_backtracking_wolfe():
    n, m = 1537, 5
    _same_as_single("rosenbrock", "backtracking_wolfe", n, m, seeds_x0(n, [1, 2, 3], -2.0, 2.0), 12, 1e-5)


# ---- 7. reuse -----------------------------------------------------------------------------------
def test_reuse_and_recreate():
    n, m, B = 513, 3, 3
    XA = seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    XB = seeds_x0(n, [4, 5, 6], -1.0, 1.0)
    runs = [("rosenbrock", XA, "backtracking", 10), ("quad_tridiag", XB, "wolfe", 8)]
    fresh = []
    for obj, X0, ls, it in runs:
        with L.Batch(n, m, B) as b:
            fresh.append(b.minimize(obj, X0, ls, max_iterations=it, trace=True))
    with L.Batch(n, m, B) as b:
        for (obj, X0, ls, it), want in zip(runs, fresh):
            got = b.minimize(obj, X0, ls, max_iterations=it, trace=True)
            assert same_bits(got["x"], want["x"]) and same_bits(got["f"], want["f"])
            assert same_bits(got["gnorm"], want["gnorm"])
            assert list(got["iterations"]) == list(want["iterations"]) and got["status"] == want["status"]
            for p in range(B):
                assert same_bits(got["tr_f"][p], want["tr_f"][p])
                assert got["events"][p] == want["events"][p]
    orc = oracle("rosenbrock", XA, "backtracking", m, 10, 1e-5, ("reuse",))
    for p in range(B):
        check_problem(fresh[0], p, orc[p], "reuse")
    for _ in range(3):
        L.Batch(n, m, B).close()


# ---- 8. refusals --------------------------------------------------------------------------------
def test_refusals():
    n, m, B = 5, 2, 3
    X0 = seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    orc = oracle("quad_sep", X0, "backtracking", m, 4, 1e-5, ("refuse",))
    for bad in [(0, 2, 1), (32769, 2, 1), (5, 0, 1), (5, 17, 1), (5, 2, 0)]:
        with pytest.raises(L.LbfgsError) as e:
            L.Batch(*bad)
        assert e.value.rc == -1
    with L.Batch(n, m, B) as b:
        def refused(**kw):
            args = dict(objective="quad_sep", X0=X0, line_search="backtracking", max_iterations=4)
            args.update(kw)
            with pytest.raises(L.LbfgsError) as e:
                b.minimize(**args)
            assert e.value.rc == -1, kw

        refused(objective="host")
        refused(objective="dense")
        for flag in (L.FLAG_VERBOSE, L.FLAG_UNFUSED, L.FLAG_VECTOR_FREE, L.FLAG_REFERENCE_CALLS,
                     L.FLAG_CUDA_COMPAT, L.FLAG_CUDA_VARIANT):
            refused(flags=flag)
        lib = L.lib()
        ev = L.BatchEvents()
        f = np.empty(8)
        for problem in (-1, B):
            assert lib.lbfgs_batch_trace_len(b.h, problem) == -1
            assert lib.lbfgs_batch_trace_get(b.h, problem, f, f, f, 8) == -1
            assert lib.lbfgs_batch_events_get(b.h, problem, ctypes.byref(ev)) == -1
        res = b.minimize("quad_sep", X0, "backtracking", max_iterations=4, trace=True)
        for p in range(B):
            check_problem(res, p, orc[p], "after refusals")
        for problem in (-1, B):
            assert lib.lbfgs_batch_trace_len(b.h, problem) == -1
            assert lib.lbfgs_batch_events_get(b.h, problem, ctypes.byref(ev)) == -1


# ---- 9. a history of 16 pairs, and of 8 -----------------------------------------------------------
@pytest.mark.parametrize("case", HC.STENCIL, ids=HC.case_id)
def test_long_history(case):
    """m = 16 (LBK_SMALL_HMAX: ring[16], sy[17], yy[17], TA[16], the spare pair in pool slot 16) and
    m = 8, on inputs that fill the ring and rotate it (tests/test_history_inputs.py asserts that on the
    CPU): the oracle's bits, and everything the single-problem path reports."""
    obj, n, m, ls, tol, differ = case
    X0, orc = HC.stencil_x0(case), HC.stencil_oracle(case)
    with L.Batch(n, m, len(X0)) as b:
        res = b.minimize(obj, X0, ls, max_iterations=HC.MAXIT, tolerance=tol, trace=True)
    with L.Context(n, m) as c:
        for p in range(len(X0)):
            check_problem(res, p, orc[p], case)
            assert [res["events"][p][k] for k in EVENT_KEYS] == message_counts(orc[p])[:4], (case, p)
            HC.check_single(res, p, c.minimize(obj, X0[p], ls, max_iterations=HC.MAXIT, tolerance=tol, trace=True), case)
    HC.check_h_max(res, orc, m, case)
    assert not differ or len(set(res["iterations"])) >= 2
