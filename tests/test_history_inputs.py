"""Conditions on the inputs of the long-history batch tests, asserted on the oracle alone (CPU).

A parity test at m = 16 passes vacuously where no problem ever stores 16 pairs. For the exact batches
the GPU tests run (tests/hist_cases.py), this file asserts what they rely on: every trace is finite,
at least two problems of every batch have iterations - skipped updates >= m + 4 (the ring fills and,
with its spare pair, rotates), and the problems of a batch end at different iterations wherever the
table says the input gives that. Where a condition fails, change the input.
"""
import numpy as np
import pytest

import hist_cases as HC


def finite(o):
    return np.all(np.isfinite(o["f"])) and np.all(np.isfinite(o["gnorm"])) and np.all(np.isfinite(o["x"]))


def check(orc, m, differ, what):
    its = [o["iters"] for o in orc]
    assert all(finite(o) for o in orc), what
    assert sum(HC.full_ring(o, m) for o in orc) >= 2, (what, its, [o["skips"] for o in orc])
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
    assert all(o["skips"] == 0 for o in HC.stencil_oracle(case)), case


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
    assert all(o["skips"] == 0 for o in orc), case


def test_history_lengths_covered():
    assert {c[2] for c in HC.STENCIL} == {8, 16} and {c[3] for c in HC.RAGGED_STENCIL} == {8, 16}
    assert {c[1] for c in HC.DENSE + HC.RAGGED_DENSE} == {16}
    assert any(c[1] < c[2] for c in HC.STENCIL)  # a history longer than the problem is wide
