"""Conditions on the inputs of tests/test_gpu_constants.py and of the varied-constants cases of
tests/devobj_gpu_cases.py and tests/batchcb_gpu_cases.py, asserted on the oracle alone (CPU).

A parity test with varied constants passes vacuously where the constants never bite. For the exact
cases the GPU tests run (tests/consts_cases.py), this file asserts everything they rely on: every
case's trace differs from the same case at the default constants and stays finite, and the
mechanisms each set is meant to reach are reached (long chains with a ratio that is no power of two,
first steps that are never accepted, steps above initial_step, the interpolation minimum and the
backtracking tolerance returned, failed searches). Where a condition fails, change the input.
"""
import os
import sys

import numpy as np
import pytest

import consts_cases as K
import oracle_lib as O


def steps(o):
    a = o["alpha"]
    return a[~np.isnan(a)]


def accepted(case, o):
    """(iterations that took initial_step, iterations that took another step)"""
    a0 = K.SETS[case[0]]["initial_step"]
    s = steps(o)
    return int(np.sum(s == a0)), int(np.sum(s != a0))


def chain_length(alpha, a0, beta, limit=200):
    """j with alpha == a0 * beta * ... * beta (j times, as the backtracking loop multiplies), or None"""
    a = a0
    for j in range(limit):
        if a == alpha:
            return j
        a *= beta
    return None


def differs(a, b):
    return not (len(a["f"]) == len(b["f"]) and np.array_equal(a["f"].view(np.uint64), b["f"].view(np.uint64))
                and np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64)))


def finite(o):
    return np.all(np.isfinite(o["f"])) and np.all(np.isfinite(o["flog"])) and np.all(np.isfinite(o["x"]))


def _id(c):
    return "-".join(str(v) for v in c)


# ---- every case: finite, and not the default constants' trace -----------------------------------
@pytest.mark.parametrize("case", K.SOLVES, ids=_id)
def test_solve_cases(case):
    o, d = K.oracle(case), K.oracle(case, default=True)
    assert finite(o) and differs(o, d)
    acc, rej = accepted(case, o)
    assert acc + rej == len(steps(o)) > 0
    ks, obj, n, m, ls, iters = case
    k = K.SETS[ks]
    if ks == "K2" and obj == "quad_tridiag":
        assert acc == 0 and rej >= 10  # every iteration recommits at another step
    if ks == "K2" and ls == "wolfe":
        assert np.any(steps(o) > k["initial_step"])
    if ks == "K3":
        # iteration 0 backtracks; every later one grows the step by 1.1 some 25 times
        assert rej == len(steps(o)) and np.sum(steps(o) > 5 * k["initial_step"]) == len(steps(o)) - 1
    if ks in ("K1", "K5") and ls == "wolfe":
        assert o["status"] == "ls_failed" and o["iters"] == 1 and "Line search failed at iteration 1" in o["messages"]
    if ks == "K4" and ls != "wolfe":
        assert o["status"] == "ls_failed" and o["iters"] == 0
    if ks == "K4" and ls == "wolfe":
        assert o["iters"] == iters and rej == iters
    if ks in ("K1", "K5") and ls != "wolfe":
        assert acc > 0 and rej > 0  # both the first step and another one are taken


def test_k1_backtracking_chains():
    """more rejections in a row than the commit's candidate plus one batched pass of four"""
    for case in K.SOLVES:
        if case[0] == "K1" and case[4] == "backtracking":
            k = K.SETS["K1"]
            js = [chain_length(a, k["initial_step"], k["backtracking_alpha"]) for a in steps(K.oracle(case))]
            assert None not in js and max(js) >= 6, (case, js)


def test_k1_wolfe_negative_step():
    case = next(c for c in K.SOLVES if c[0] == "K1" and c[4] == "wolfe")
    assert np.any(steps(K.oracle(case)) < 0)


def test_k5_limits_are_returned():
    k = K.SETS["K5"]
    interp = next(c for c in K.SOLVES if c[0] == "K5" and c[4] == "interpolation")
    assert np.any(steps(K.oracle(interp)) == k["wolfe_interp_min"])
    bt = next(c for c in K.SOLVES if c[0] == "K5" and c[4] == "backtracking")
    assert np.any(steps(K.oracle(bt)) < k["backtracking_tol"] / k["backtracking_alpha"])


@pytest.mark.parametrize("case", K.VECTOR_FREE, ids=_id)
def test_vector_free_cases(case):
    o, d = K.oracle(case, vector_free=True), K.oracle(case, default=True, vector_free=True)
    assert finite(o) and differs(o, d)
    acc, rej = accepted(case, o)
    assert rej > 0 and (case[0] != "K2" or acc == 0)


@pytest.mark.parametrize("case", K.UNFUSED, ids=_id)
def test_unfused_cases(case):
    o, d = K.oracle(case), K.oracle(case, default=True)
    assert finite(o) and differs(o, d)


@pytest.mark.parametrize("cuda", [1, 2])
@pytest.mark.parametrize("case", K.CUDA_COMPAT, ids=_id)
def test_cuda_compat_cases(case, cuda):
    """against the CUDA profile (c2 = 0.7), which is what those loops have been run with so far"""
    o, d = K.oracle(case, cuda=cuda), K.oracle(case, default=True, cuda=cuda)
    assert finite(o)
    # a search with the file's own constants must NOT follow lbfgs_constants: the parity test then
    # shows that the device ignores them there too
    assert differs(o, d) == ((cuda, case[4]) not in K.CUDA_OWN_CONSTANTS)


@pytest.mark.parametrize("case", K.HOST + K.DENSE, ids=_id)
def test_external_objective_cases(case):
    o, d = K.oracle(case), K.oracle(case, default=True)
    assert finite(o) and differs(o, d)
    assert accepted(case, o)[1] > 0


@pytest.mark.parametrize("case", K.BATCH_STENCIL, ids=_id)
def test_batch_stencil_cases(case):
    for seed in K.BATCH_SEEDS:
        o, d = K.oracle(case, seed=seed), K.oracle(case, seed=seed, default=True)
        assert finite(o) and differs(o, d), seed


@pytest.mark.parametrize("case", K.BATCH_DENSE, ids=_id)
def test_batch_dense_cases(case):
    for q in K.BATCH_DENSE_Q:
        o, d = K.oracle(case, seed=10 + q, dense_q=q), K.oracle(case, seed=10 + q, dense_q=q, default=True)
        assert finite(o) and differs(o, d), q


@pytest.mark.parametrize("case", K.DEVICE_OBJ, ids=_id)
def test_device_objective_cases(case):
    """path 11: the objective as callables, as the device callback evaluates it"""
    o, d = K.oracle(case, host=True), K.oracle(case, host=True, default=True)
    assert finite(o) and differs(o, d)
    assert accepted(case, o)[1] > 0


@pytest.mark.parametrize("case", K.BATCH_CALLBACK, ids=_id)
def test_batch_callback_cases(case):
    """path 12. Three of the four starts or more leave the default constants' run (the start at the
    minimiser takes the default steps under K1 / K5 + Wolfe at n = 513, the scaled one under K1 +
    interpolation at n = 5), and each entry reaches what its comment in consts_cases.py says."""
    ks, obj, n, m, ls, iters = case
    k = K.SETS[ks]
    runs = [K.oracle(case, host=True, x0=x0) for x0 in K.batch_x0(n)]
    dflt = [K.oracle(case, host=True, x0=x0, default=True) for x0 in K.batch_x0(n)]
    assert all(finite(o) for o in runs)
    assert sum(differs(o, d) for o, d in zip(runs, dflt)) >= 3
    failed = [o["status"] == "ls_failed" for o in runs]
    if ks in ("K1", "K5") and ls == "wolfe":  # a mixed batch: three fail at iteration 1, one runs on
        assert [o["iters"] for o in runs if o["status"] == "ls_failed"] == [1, 1, 1] and sum(failed) == 3
        assert [o["iters"] for o in runs if o["status"] != "ls_failed"] == [iters]
    elif ks == "K2" and ls == "wolfe":  # expands above initial_step in every iteration of every problem
        assert all(np.all(steps(o) > k["initial_step"]) and o["iters"] == iters for o in runs)
        assert all(o["nf_total"] >= 20 * iters for o in runs)
    elif ks == "K3" and ls == "backtracking_wolfe":  # the step grows by 1.1 some 24 times per search, two f values a trial
        assert all(o["iters"] == iters and o["nf_total"] >= 40 * iters for o in runs)
        assert all(np.sum(steps(o) > 5 * k["initial_step"]) >= iters - 1 for o in runs)
    elif ks == "K3" and ls == "wolfe":  # problems that end inside their first search, beside one that runs on
        assert sorted(o["iters"] for o in runs) == [0, 0, 0, iters] and sum(failed) == 3
    elif ks == "K4":  # fails at once
        assert all(failed) and all(o["iters"] == 0 for o in runs)
    else:
        assert not any(failed) and all(accepted(case, o)[1] > 0 for o in runs)
    if ks == "K2" and ls != "wolfe":
        assert all(accepted(case, o)[0] == 0 for o in runs)  # no first step accepted


def test_long_search_case():
    """backtracking_alpha = 0.99: the middle row's first search rejects 300 steps or more, the rows
    beside it converge at their first evaluation"""
    c = K.LONG_SEARCH
    runs = [O.lbfgs(c["objective"], x0, c["search"], c["m"], c["iterations"], K.TOL, mode=O.CANON, consts=c["consts"])
            for x0 in K.long_search_x0()]
    for p, o in enumerate(runs):
        if p == c["row"]:
            j = chain_length(o["alpha"][0], 1.0, c["consts"]["backtracking_alpha"], limit=2000)
            assert j is not None and j >= c["rejected_at_least"], (o["alpha"], j)
            assert o["iters"] == c["iterations"] and finite(o)
        else:
            assert o["iters"] == 0 and o["status"] == "converged"


@pytest.mark.parametrize("case", K.BATCH_RAGGED + K.BATCH_RAGGED_DENSE, ids=K.ragged_id)
def test_batch_ragged_cases(case):
    """path 13: every problem of every batch, at its own size"""
    subs = K.ragged_problems(case)
    assert len({s[0][2] for s in subs}) >= 2  # sizes differ within the batch
    for sub, kw in subs:
        o, d = K.oracle(sub, **kw), K.oracle(sub, default=True, **kw)
        assert finite(o) and differs(o, d), (sub, kw)


@pytest.mark.parametrize("ks,ls", K.LINE_SEARCH)
def test_line_search_cases(ks, ls):
    """the step of iteration 0 from the point is not the default constants' step. (Along -g the Wolfe
    search has its step before c1 = 0.3 / c2 = 0.5 decide otherwise than 1e-4 / 0.9, from every point
    tried: K1 and K5 + Wolfe check only that initial_step is not taken.)"""
    case = (ks, "rosenbrock", K.LS_N, 2, ls, 1)
    o, d = K.oracle(case, seed=K.LS_SEED), K.oracle(case, seed=K.LS_SEED, default=True)
    assert finite(o) and np.isfinite(o["alpha"][0])
    assert o["alpha"][0] != K.SETS[ks]["initial_step"]  # the first step was rejected
    if (ks, ls) not in (("K1", "wolfe"), ("K5", "wolfe")):
        assert o["alpha"][0] != d["alpha"][0]


def test_sharded_case():
    ks, obj, n, m, ls, iters = K.SHARDED
    # (the oracle at n = 70 001 stands in for 2.1e6 here; the GPU test asserts on its own one-rank
    # run that steps above initial_step are taken)
    small = (ks, obj, 70_001, m, ls, iters)
    o, d = K.oracle(small), K.oracle(small, default=True)
    assert finite(o) and differs(o, d) and np.any(steps(o) > K.SETS[ks]["initial_step"])
    sys.path.insert(0, os.path.join(O.ROOT, "cuda-lbfgs_amd"))
    import lbfgs_amd as L

    assert all(L.shard_range(n, r, 2)[1] > 0 for r in range(2))  # every rank owns segments
