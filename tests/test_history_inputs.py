"""Conditions on the inputs of the long-history tests, asserted on the oracle alone (CPU).

A parity test at m = 16 passes vacuously where no problem ever stores 16 pairs. For the exact batches
the GPU tests run (tests/hist_cases.py), this file asserts what they rely on: every trace is finite,
at least two problems of every batch have iterations - skipped updates >= m + 4 (the ring fills and,
with its spare pair, rotates), and the problems of a batch end at different iterations wherever the
table says the input gives that. Skipped updates are counted from the oracle's "Skipping update"
lines (hist_cases.skipped_updates), and every case's counts are stated. The single-problem cases with
17 to 64 pairs (SINGLE_LONG, tests/test_gpu_long_history.py) come last, with the two-loop primitive's
bound against a long-double recursion. Where a condition fails, change the input.
"""
import numpy as np
import pytest

import hist_cases as HC


def finite(o):
    return np.all(np.isfinite(o["f"])) and np.all(np.isfinite(o["gnorm"])) and np.all(np.isfinite(o["x"]))


def check(orc, m, differ, what):
    its = [o["iters"] for o in orc]
    assert all(finite(o) for o in orc), what
    assert sum(HC.full_ring(o, m) for o in orc) >= 2, (what, its, [HC.skipped_updates(o) for o in orc])
    if differ:
        assert len(set(its)) >= 2, (what, its)
    return its


@pytest.mark.parametrize("host", [False, True], ids=["builtin", "callables"])
@pytest.mark.parametrize("case", HC.STENCIL, ids=HC.case_id)
def test_stencil_batches(case, host):
    """the uniform stencil batch's inputs, and the callback batch's (the objective as callables)"""
    obj, n, m, ls, tol, differ = case
    its = check(HC.stencil_oracle(case, HC.Callables if host else None), m, differ, case)
    if obj == "rosenbrock":  # every problem fills the ring of 16 (the start at the minimiser: n >= 17)
        assert all(k >= (m + 4 if n >= 17 else m + 3) for k in its), its
        assert sum(k >= 2 * m + 4 for k in its) >= 3, its  # three of the four rotate the whole ring once more
    # none skipped, except the scaled start at n = 5 (hist_cases.STENCIL_SKIPS, with which full_ring holds)
    orc = HC.stencil_oracle(case, HC.Callables if host else None)
    assert [HC.skipped_updates(o) for o in orc] == HC.stencil_skips(case), case
    if any(HC.stencil_skips(case)):
        assert [HC.full_ring(o, m) for o in orc] == [True, True, False, True], case


def test_callables_give_the_builtin_objectives_bits():
    for case in HC.STENCIL:
        for a, b in zip(HC.stencil_oracle(case), HC.stencil_oracle(case, HC.Callables)):
            assert np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64)) and a["iters"] == b["iters"], case


@pytest.mark.parametrize("case", HC.RAGGED_STENCIL, ids=HC.case_id)
def test_ragged_stencil_batches(case):
    obj, sizes, starts, m, ls, tol, differ = case
    assert len(set(sizes)) == len(sizes) >= 3  # m = 16 meets problems of different sizes
    check(HC.stencil_oracle(case), m, differ, case)


@pytest.mark.parametrize("case", HC.DENSE + HC.RAGGED_DENSE, ids=HC.case_id)
def test_dense_batches(case):
    n, m, ls = case
    orc = HC.dense_oracle(case)
    its = check(orc, m, True, case)
    assert max(its) == HC.MAXIT and min(its) >= m + 1, its  # the early problem too reaches h = m
    assert all(HC.skipped_updates(o) == 0 for o in orc), case


def test_history_lengths_covered():
    assert {c[2] for c in HC.STENCIL} == {8, 16} and {c[3] for c in HC.RAGGED_STENCIL} == {8, 16}
    assert {c[1] for c in HC.DENSE + HC.RAGGED_DENSE} == {16}
    assert any(c[1] < c[2] for c in HC.STENCIL)  # a history longer than the problem is wide


def test_skipped_updates_counts_the_standard_paths_lines():
    """the oracle's "skips" field is the CUDA path's and stays 0 on the standard path, whatever it skips"""
    o = HC.stencil_oracle(("rosenbrock", 5, 16, "backtracking", 1e-7, True))[1]
    assert o["skips"] == 0 and HC.skipped_updates(o) == 19 == o["messages"].count("Skipping update")


# ---- 17 to 64 pairs on the single-problem paths ----
@pytest.mark.parametrize("case", HC.SINGLE_LONG + HC.SINGLE_LONG_LARGE, ids=HC.long_id)
def test_single_long_cases(case):
    """every run is finite, ends at its iteration limit, skips what the table says, stores m pairs and
    rotates the ring through at least 4 more, the cases of SINGLE_LONG through at least 12 more"""
    n, m, ls, it = case
    o = HC.long_oracle(case)
    assert finite(o), case
    assert o["status"] == "max_iter" and o["iters"] == it, (case, o["status"], o["iters"])
    assert o["messages"].strip().splitlines()[-1] == "Maximum iterations reached"
    assert HC.skipped_updates(o) == HC.LONG_SKIPS.get(case, 0), (case, HC.skipped_updates(o))
    assert HC.full_ring(o, m), case
    if case in HC.SINGLE_LONG:
        assert o["iters"] - HC.skipped_updates(o) >= m + 12, case
    if m == 64:  # some line search goes past its first trial while more than 16 pairs are stored
        assert len(HC.late_searches(o)) >= (4 if n <= 1537 else 3), (case, HC.late_searches(o))


def test_single_long_table():
    assert len(HC.SINGLE_LONG) == 36 and len(set(HC.SINGLE_LONG)) == 36
    assert {(c[1], c[3]) for c in HC.SINGLE_LONG} == set(HC.LONG_M) == {(17, 30), (24, 40), (64, 80)}
    assert {c[0] for c in HC.SINGLE_LONG} == {17, 513, 1537} and {c[2] for c in HC.SINGLE_LONG} == set(HC.SEARCHES)
    assert set(HC.LONG_SKIPS) <= set(HC.SINGLE_LONG)
    assert all(c[1] > 16 for c in HC.SINGLE_LONG + HC.SINGLE_LONG_LARGE)
    assert len(HC.LONG_DEVICE_SEARCH) == 26 and set(HC.LONG_DEVICE_SEARCH) <= set(HC.SINGLE_LONG)
    assert {c[2] for c in HC.LONG_DEVICE_SEARCH} == set(HC.SEARCHES)


@pytest.mark.parametrize("ls", HC.SEARCHES)
@pytest.mark.parametrize("n", HC.LONG_N)
def test_single_long_searches_past_the_first_trial(n, ls):
    """for every n and search some m has an iteration k >= 18 whose step is not the initial step; m = 17
    has one everywhere but at (17, interpolation), m = 24 lacks one for three searches at n = 513"""
    late = {m: HC.late_searches(HC.long_oracle((n, m, ls, it))) for m, it in HC.LONG_M}
    assert any(late.values()), (n, ls)
    assert bool(late[64]) and bool(late[17]) == ((n, ls) != (17, "interpolation")), (n, ls, late)
    assert bool(late[24]) == (n != 513 or ls == "wolfe"), (n, ls, late)


@pytest.mark.parametrize("cuda", [1, 2])
@pytest.mark.parametrize("ls", HC.SEARCHES)
def test_single_long_cuda_path_runs(ls, cuda):
    """the CUDA path's loops at m = 64: finite, and past iteration 64, where the slot k % m wraps"""
    o = HC.long_cuda_oracle(ls, cuda)
    assert finite(o) and o["iters"] >= 64 + 12, (ls, cuda, o["iters"], o["status"])


# ---- the two-loop primitive against the same recursion in long double ----
@pytest.mark.parametrize("h,n", HC.TWOLOOP_LONG)
def test_oracle_twoloop_within_bound_of_long_double(h, n):
    """the bound test_gpu_parity.py asserts for the device two-loop holds for the oracle alone"""
    g, S, Y = HC.twoloop_inputs(h, n)
    d, _ = HC.O.twoloop(g, S, Y, HC.O.CANON)
    err = HC.twoloop_error(d, HC.twoloop_longdouble(g, S, Y))
    assert err <= HC.TWOLOOP_BOUND, (h, n, err)
