"""GPU tests of ragged batches (lbfgs_batch_create_ragged, L.Batch with a list of sizes): B problems of
different sizes in one batch, one workgroup each, packed storage, a per-problem table in device
memory. Everything is compared bit for bit, never a tolerance: the feature moves data, not
arithmetic. The reference is the canonical-order oracle run once per problem on the CPU at that
problem's own n_p (for dense after O.dense_set(A_p, b_p)).

Sizes are the smallest at which each mechanism can go wrong: 513 (a second segment of one element),
5 (one partial row), 1537 (four segments, the last of one element), 512 (exactly one segment), 129
(one row of a wave plus one element), 1024 (two full segments), 32768 beside 5 (64 segments beside
one: every lane of the stage-2 wave live for one problem and one lane for the next); m = 16 and 8 with
sizes [1537, 17, 513] (stencil) and [513, 65, 100] (dense), 40 iterations at most: the largest history a
batch accepts, filled and rotated beside problems of other sizes (tests/hist_cases.py)."""
import ctypes as C
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
SIZES = [513, 5, 1537, 512, 129, 1024]
COUNTERS = ("f", "gnorm", "iterations", "status_code", "trials_f", "trials_fg", "commits", "h_min", "h_max", "bytes")
BAD_ARG = -1


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    """Equal bit for bit; a NaN equals a NaN in the same place (its sign and payload are the
    processor's: x86 and the GPU produce different ones from the same operation)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def message_counts(o):
    return [sum(1 for line in o["messages"].splitlines() if m in line) for m in MESSAGES]


def check_problem(res, p, o, what=""):
    """x, f, |g|, iterations, status, the traces and the event counts of problem p against its oracle
    run (after a failed line search the result's f is f at the failed step, which the oracle does not
    return)."""
    assert res["status"][p] == o["status"], (what, p, res["status"][p], o["status"])
    assert res["iterations"][p] == o["iters"], (what, p, res["iterations"][p], o["iters"])
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
    want = message_counts(o)
    assert [res["events"][p][k] for k in EVENT_KEYS] == want[:4], (what, p, res["events"][p], want)
    assert (res["status"][p] == "ls_failed") == (want[4] > 0), (what, p)


def same_results(ra, pa, rb, pb, what):
    """problem pa of one result against problem pb of another: everything the library reports"""
    assert same_bits(ra["x"][pa], rb["x"][pb]), (what, pa, pb)
    for k in COUNTERS:
        assert same_bits([float(ra[k][pa])], [float(rb[k][pb])]), (what, k, pa, pb, ra[k][pa], rb[k][pb])
    for k in ("tr_f", "tr_gnorm", "tr_alpha"):
        assert same_bits(ra[k][pa], rb[k][pb]), (what, k, pa, pb)
    assert ra["events"][pa] == rb["events"][pb], (what, pa, pb)


def x0s(sizes, lo=-2.0, hi=2.0, seed0=1):
    return [O.x0_uniform(n, seed0 + p, lo, hi) for p, n in enumerate(sizes)]


_oracle = {}


def oracle(key, obj, X0, ls, m, maxit, tol):
    """The oracle's runs of a batch, each at its own size, computed once per key and shared (left unchanged)."""
    if key not in _oracle:
        _oracle[key] = [O.lbfgs(obj, x0, ls, m, maxit, tol, mode=O.CANON) for x0 in X0]
    return _oracle[key]


def solve(sizes, m, obj, X0, ls, maxit, tol=1e-5, launch=None):
    with L.Batch(sizes, m) as b:
        assert b.ragged and b.sizes == list(sizes) and b.n == max(sizes) and b.batch == len(sizes)
        assert b.offsets == [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]
        if launch:
            b.set_launch(*launch)
        return b.minimize(obj, X0, ls, max_iterations=maxit, tolerance=tol, trace=True)


# ---- 1. parity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("ls", SEARCHES)
@pytest.mark.parametrize("obj", OBJS)
def test_parity(obj, ls, m):
    X0 = x0s(SIZES)
    orc = oracle(("parity", obj, ls, m), obj, X0, ls, m, 12, 1e-5)
    res = solve(SIZES, m, obj, X0, ls, 12)
    assert isinstance(res["x"], list) and [len(x) for x in res["x"]] == SIZES
    for p in range(len(SIZES)):
        check_problem(res, p, orc[p], (obj, ls, m))
        assert res["bytes"][p] > 0 and res["bytes"][p] % (8 * SIZES[p]) == 0  # counted with n_p


def test_bytes_and_counters_are_those_of_each_problem_at_its_own_size():
    """Every counter of problem p, bytes among them, against a uniform batch of that one problem at n_p
    (whose bytes count n_p): a count with the largest size would differ in all but one problem."""
    m, ls = 5, "backtracking"
    X0 = x0s(SIZES)
    res = solve(SIZES, m, "rosenbrock", X0, ls, 12)
    out = np.full(sum(SIZES), np.nan)
    with L.Batch(SIZES, m) as b:
        again = b.minimize("rosenbrock", np.concatenate(X0), ls, max_iterations=12, tolerance=1e-5, trace=True, out=out)
        with pytest.raises(ValueError):
            b.minimize("rosenbrock", X0, ls, max_iterations=12, out=out[:-1])
        with pytest.raises(TypeError):
            b.minimize("rosenbrock", X0, ls, max_iterations=12, out=out.astype(np.float32))
    assert again["x"][0].base is out or np.shares_memory(again["x"][0], out)
    for p, n in enumerate(SIZES):
        with L.Batch(n, m, 1) as one:
            r1 = one.minimize("rosenbrock", X0[p][None, :], ls, max_iterations=12, tolerance=1e-5, trace=True)
        same_results(res, p, r1, 0, ("own size", n))
        same_results(again, p, r1, 0, ("own size, packed in and out", n))
    assert len(set(res["bytes"] / res["bytes"][0])) > 1
    with L.Batch(np.array(5), 2, np.array(2)) as b:  # a 0-d array is one size, a uniform batch
        assert not b.ragged and b.sizes == [5, 5]


# ---- 2. extremes ----------------------------------------------------------------------------------
def test_64_segments_beside_one():
    sizes = [32768, 5]
    assert O.geometry(32768) == (512, 64) and O.geometry(5)[1] == 1
    X0 = x0s(sizes)
    orc = oracle(("extremes",), "rosenbrock", X0, "backtracking", 3, 6, 1e-5)
    for launch in (None, (1, 0)):  # side by side, and one workgroup taking both in turn
        res = solve(sizes, 3, "rosenbrock", X0, "backtracking", 6, launch=launch)
        for p in range(2):
            check_problem(res, p, orc[p], ("extremes", launch))


# ---- 3. one workgroup shrinks and grows ---------------------------------------------------------------
def test_shrinking_and_growing_on_one_workgroup():
    sizes, m = [1537, 5, 32768, 5, 513], 3
    X0 = x0s(sizes)
    orc = oracle(("shrink",), "rosenbrock", X0, "interpolation", m, 8, 1e-5)
    assert all(o["iters"] == 8 for o in orc)  # a condition on the inputs (CPU): re-entries from a stored record
    base = solve(sizes, m, "rosenbrock", X0, "interpolation", 8)
    for p in range(len(sizes)):
        check_problem(base, p, orc[p], "default launch")
    with L.Batch(sizes, m) as b:
        for wg in (1, 2):
            for ipl in (1, 3, 64):
                b.set_launch(max_workgroups=wg, iters_per_launch=ipl)
                res = b.minimize("rosenbrock", X0, "interpolation", max_iterations=8, tolerance=1e-5, trace=True)
                assert (res["launches"] > 1) == (ipl < 8), (wg, ipl, res["launches"])
                for p in range(len(sizes)):
                    check_problem(res, p, orc[p], (wg, ipl))
                    same_results(res, p, base, p, (wg, ipl))


# ---- 4. all sizes equal -------------------------------------------------------------------------------
@pytest.mark.parametrize("obj,ls", [("rosenbrock", "backtracking"), ("quad_tridiag", "wolfe")])
def test_all_sizes_equal_is_the_uniform_batch(obj, ls):
    n, m, B = 513, 3, 4
    X0 = x0s([n] * B)
    rag = solve([n] * B, m, obj, X0, ls, 10)
    with L.Batch(n, m, B) as b:
        assert not b.ragged and b.sizes == [n] * B and b.offsets == [p * n for p in range(B + 1)]
        uni = b.minimize(obj, np.stack(X0), ls, max_iterations=10, tolerance=1e-5, trace=True)
    for p in range(B):
        same_results(rag, p, uni, p, (obj, ls))


# ---- 5. order does not matter -------------------------------------------------------------------------
def _forty():
    B = 40
    sizes = [SIZES[p % len(SIZES)] for p in range(B)]
    return sizes, x0s(sizes)


def _solve_forty(sizes, X0):
    return solve(sizes, 3, "rosenbrock", X0, "backtracking", 6, launch=(3, 0))


@pytest.fixture(scope="module")
def forty():
    sizes, X0 = _forty()
    return sizes, X0, _solve_forty(sizes, X0)


def test_permuting_the_problems_permutes_the_results(forty):
    sizes, X0, base = forty
    perm = np.random.RandomState(5).permutation(len(sizes))
    assert not np.array_equal(perm, np.arange(len(sizes)))
    res = _solve_forty([sizes[q] for q in perm], [X0[q] for q in perm])
    for i, q in enumerate(perm):
        same_results(res, i, base, int(q), "permuted")
    for p in (0, 1, 2, 38, 39):  # and the batch is right, not only consistent
        check_problem(base, p, O.lbfgs("rosenbrock", X0[p], "backtracking", 3, 6, 1e-5, mode=O.CANON), "B=40")


def test_work_order_forced_to_identity(forty, monkeypatch):
    """The order of work (largest problems first) against LBFGS_BATCH_ORDER=identity, read at creation."""
    sizes, X0, base = forty
    monkeypatch.setenv("LBFGS_BATCH_ORDER", "identity")
    res = _solve_forty(sizes, X0)
    for p in range(len(sizes)):
        same_results(res, p, base, p, "identity order")


# ---- 6. problems end at different times ------------------------------------------------------------------
def test_problems_end_at_different_times():
    sizes, m = [513, 5, 1024], 3
    X0 = [O.x0_uniform(513, 3, -30.0, 30.0), np.zeros(5), 1.0 + O.x0_uniform(1024, 4, -1e-4, 1e-4)]
    orc = oracle(("ends",), "quad_tridiag", X0, "wolfe", m, 25, 1e-5)
    iters = [o["iters"] for o in orc]
    assert 0 in iters and len(set(iters)) >= 3, iters  # a condition on the inputs (CPU)
    for launch in (None, (1, 2)):
        res = solve(sizes, m, "quad_tridiag", X0, "wolfe", 25, launch=launch)
        for p in range(3):
            check_problem(res, p, orc[p], ("ends", launch))
        assert list(res["iterations"]) == iters
    # the other starts of the uniform batch's test: ones, and a narrow uniform at the smallest size
    X1 = [np.ones(513), 1.0 + O.x0_uniform(5, 4, -1e-4, 1e-4), O.x0_uniform(1024, 2, -1e-3, 1e-3)]
    orc1 = oracle(("ends", 1), "quad_tridiag", X1, "wolfe", m, 25, 1e-5)
    res = solve(sizes, m, "quad_tridiag", X1, "wolfe", 25)
    for p in range(3):
        check_problem(res, p, orc1[p], "ends, second starts")


# ---- 7. guard paths --------------------------------------------------------------------------------------
GUARDS = [  # (objective, line search, m, lo, hi, max_iterations, tol, the messages the row is to reach)
    ("rosenbrock", "wolfe", 5, -1e-3, 1e-3, 60, 0.0, [4]),
    ("rosenbrock", "backtracking", 5, -1e-3, 1e-3, 60, 0.0, [0, 1]),
]


@pytest.mark.parametrize("case", GUARDS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_guard_paths(case):
    obj, ls, m, lo, hi, maxit, tol, reach = case
    sizes = [5, 129] * 3
    X0 = [O.x0_uniform(n, 1 + p // 2, lo, hi) for p, n in enumerate(sizes)]
    orc = oracle(("guard", obj, ls), obj, X0, ls, m, maxit, tol)
    total = np.sum([message_counts(o) for o in orc], axis=0)
    assert all(total[k] > 0 for k in reach), dict(zip(MESSAGES, total))  # a condition on the inputs (CPU)
    res = solve(sizes, m, obj, X0, ls, maxit, tol)
    for p in range(len(sizes)):
        check_problem(res, p, orc[p], case)
        if res["status"][p] == "ls_failed":  # f at the failed step: the single-problem path's
            with L.Context(sizes[p], m) as c:
                one = c.minimize(obj, X0[p], ls, max_iterations=maxit, tolerance=tol)
            assert one["status"] == "ls_failed" and same_bits([res["f"][p]], [one["f"]]), (case, p)


# ---- 8. dense ---------------------------------------------------------------------------------------------
DSIZES = [2, 3, 64, 65, 100, 513]


def spd(n, seed):
    """A with the eigenvalues 1 ... 1000 (logarithmically spaced) in a random orthogonal basis,
    symmetrised; b and x0 random."""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    M = (Q * np.logspace(0, 3, n)) @ Q.T
    return (M + M.T) / 2, rs.uniform(-1.0, 1.0, n), O.x0_uniform(n, seed, -2.0, 2.0)


def dense_data(scale=1.0):
    A, b, X0 = zip(*[spd(n, 3000 + n) for n in DSIZES])
    return [scale * a for a in A], [scale * v for v in b], list(X0)


def dense_oracle(key, A, b, X0, ls, m, maxit):
    if key not in _oracle:
        runs = []
        for p in range(len(X0)):
            O.dense_set(A[p], b[p])
            runs.append(O.lbfgs("dense", X0[p], ls, m, maxit, 1e-5, mode=O.CANON))
        _oracle[key] = runs
    return _oracle[key]


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("ls", SEARCHES)
def test_dense_parity(ls, m):
    A, b, X0 = dense_data()
    orc = dense_oracle(("dense", ls, m), A, b, X0, ls, m, 14)
    assert any(o["iters"] == 14 > m + 2 for o in orc)  # a condition on the inputs (CPU): the ring rotates
    with L.Batch(DSIZES, m) as bt:
        bt.set_dense_quadratics(A, b)
        res = bt.minimize("dense", X0, ls, max_iterations=14, tolerance=1e-5, trace=True)
    for p in range(len(DSIZES)):
        check_problem(res, p, orc[p], ("dense", ls, m))
        assert res["bytes"][p] % (8 * DSIZES[p]) == 0


def test_dense_counters_replaced_data_and_a_stencil_solve_after():
    m, ls = 5, "wolfe"
    A1, b1, X0 = dense_data()
    A2 = [0.5 * a + 0.5 * np.eye(len(a)) for a in A1]
    b2 = [2.0 * v for v in b1]
    orc1 = dense_oracle(("dense", ls, m), A1, b1, X0, ls, m, 14)
    orc2 = dense_oracle(("dense2", ls, m), A2, b2, X0, ls, m, 14)
    sten = x0s(DSIZES, seed0=7)
    orc3 = oracle(("dense-stencil",), "quad_tridiag", sten, "backtracking", m, 6, 1e-5)
    with L.Batch(DSIZES, m) as bt:
        bt.set_dense_quadratics(A1, b1)
        first = bt.minimize("dense", X0, ls, max_iterations=14, tolerance=1e-5, trace=True)
        bt.set_dense_quadratics(np.concatenate([a.ravel() for a in A2]), np.concatenate(b2))  # packed arrays
        second = bt.minimize("dense", X0, ls, max_iterations=14, tolerance=1e-5, trace=True)
        # the stencil halo loads rely on zero ghosts and padding, also of the packed neighbours
        stencil = bt.minimize("quad_tridiag", sten, "backtracking", max_iterations=6, tolerance=1e-5, trace=True)
        again = bt.minimize("dense", X0, ls, max_iterations=14, tolerance=1e-5, trace=True)
    for p in range(len(DSIZES)):
        check_problem(first, p, orc1[p], "first data")
        check_problem(second, p, orc2[p], "second data")
        check_problem(stencil, p, orc3[p], "stencil after dense")
        same_results(again, p, second, p, "dense after stencil")
        with L.Batch(DSIZES[p], m, 1) as one:  # bytes and every other counter: the problem alone at its own size
            one.set_dense_quadratics(A1[p][None], b1[p][None])
            r1 = one.minimize("dense", X0[p][None, :], ls, max_iterations=14, tolerance=1e-5, trace=True)
        same_results(first, p, r1, 0, ("dense, own size", p))
    for p in (3, 5):  # n = 65 and 513: the single-problem path's counters
        with L.Context(DSIZES[p], m) as c:
            c.set_dense_quadratic(A1[p], b1[p])
            one = c.minimize("dense", X0[p], ls, max_iterations=14, tolerance=1e-5, trace=True)
        assert same_bits(first["x"][p], one["x"]) and same_bits(first["tr_f"][p], one["tr_f"]), p
        for k in ("trials_f", "trials_fg", "commits", "h_min", "h_max", "iterations"):
            assert first[k][p] == one[k], (p, k, first[k][p], one[k])


# ---- 8b. a history of 16 pairs, and of 8, beside problems of other sizes -------------------------------------
def _single(n, m, obj, x0, ls, tol, dense=None):
    with L.Context(n, m) as c:
        if dense is not None:
            c.set_dense_quadratic(*dense)
        return c.minimize(obj, x0, ls, max_iterations=HC.MAXIT, tolerance=tol, trace=True)


@pytest.mark.parametrize("case", HC.RAGGED_STENCIL, ids=HC.case_id)
def test_long_history(case):
    """m = 16 (the largest history a batch accepts) and m = 8 with sizes [1537, 17, 513] in one batch, on
    inputs that fill the ring and rotate it (tests/test_history_inputs.py asserts that on the CPU): the
    oracle's bits, and everything one single-problem solve per problem reports."""
    obj, sizes, starts, m, ls, tol, differ = case
    X0, orc = HC.ragged_x0(case), HC.stencil_oracle(case)
    res = solve(sizes, m, obj, X0, ls, HC.MAXIT, tol)
    for p, n in enumerate(sizes):
        check_problem(res, p, orc[p], case)
        HC.check_single(res, p, _single(n, m, obj, X0[p], ls, tol), case)
    HC.check_h_max(res, orc, m, case)
    assert len(set(res["iterations"])) >= 2


@pytest.mark.parametrize("case", HC.RAGGED_DENSE, ids=HC.case_id)
def test_dense_long_history(case):
    """the same in the dense kernels: sizes [513, 65, 100], m = 16, 40 iterations at most"""
    sizes, m, ls = case
    A, b, X0 = HC.ragged_dense_data()
    orc = HC.dense_oracle(case)
    with L.Batch(list(sizes), m) as bt:
        bt.set_dense_quadratics(A, b)
        res = bt.minimize("dense", X0, ls, max_iterations=HC.MAXIT, tolerance=HC.DENSE_TOL, trace=True)
    for p, n in enumerate(sizes):
        check_problem(res, p, orc[p], case)
        HC.check_single(res, p, _single(n, m, "dense", X0[p], ls, HC.DENSE_TOL, dense=(A[p], b[p])), case)
    HC.check_h_max(res, orc, m, case)
    assert len(set(res["iterations"])) >= 2


# ---- 9. refusals ------------------------------------------------------------------------------------------
def test_refusals():
    sizes, m = [5, 129, 2], 2
    X0 = x0s(sizes)
    orc = oracle(("refuse",), "quad_sep", X0, "backtracking", m, 4, 1e-5)
    lib = L.lib()
    for bad in ([5, 0], [5, 32769], []):
        with pytest.raises((L.LbfgsError, ValueError)):
            L.Batch(bad, m)
    with pytest.raises(ValueError):
        L.Batch(sizes, m, batch=2)
    with L.Batch(sizes, m) as bt:
        for bad in (X0[:2], X0 + [X0[0]], [X0[0], X0[1][:100], X0[2]], np.concatenate(X0)[:-1],
                    np.zeros((3, 129))):
            with pytest.raises(ValueError):
                bt.minimize("quad_sep", bad, "backtracking", max_iterations=4)
        A = [np.eye(n) for n in sizes]
        b = [np.zeros(n) for n in sizes]
        with pytest.raises(ValueError):
            bt.set_dense_quadratics(A[:2], b)
        with pytest.raises(ValueError):
            bt.set_dense_quadratics(A, [b[0], b[1]])
        with pytest.raises(ValueError):
            bt.set_dense_quadratics(np.eye(129), b)  # one shared matrix: not on a ragged batch
        packed_A = np.concatenate([a.ravel() for a in A])
        packed_b = np.concatenate(b)
        rc = lib.lbfgs_batch_set_dense_quadratics(bt.h, packed_A.ctypes.data_as(C.c_void_p), 1,
                                                  packed_b.ctypes.data_as(C.c_void_p))
        assert rc == BAD_ARG and b"ragged" in lib.lbfgs_batch_last_error(bt.h)
        with pytest.raises(L.LbfgsError) as e:  # a refused setter sets nothing
            bt.minimize("dense", X0, "backtracking", max_iterations=4)
        assert e.value.rc == BAD_ARG
        res = bt.minimize("quad_sep", X0, "backtracking", max_iterations=4, trace=True)  # the object still solves
        for p in range(len(sizes)):
            check_problem(res, p, orc[p], "after refusals")
    big = [5, L.DENSE_BATCH_NMAX + 1]
    with L.Batch(big, 1) as bt:  # a batch the stencil objectives can use, one problem over the dense limit
        with pytest.raises(L.LbfgsError) as e:
            bt.set_dense_quadratics([np.eye(n) for n in big], [np.zeros(n) for n in big])
        assert e.value.rc == BAD_ARG
        xb = x0s(big)
        res = bt.minimize("quad_sep", xb, "backtracking", max_iterations=2, trace=True)
        for p in range(2):
            check_problem(res, p, O.lbfgs("quad_sep", xb[p], "backtracking", 1, 2, 1e-5, mode=O.CANON), "big")
    # LBFGS_BATCH_PACKED is a stride of ragged batches only (the C level; the pointers are the batch's
    # own business: the strides are refused before any pointer is looked at)
    with L.Batch(5, m, 3) as bt:
        k = L.constants()
        r3 = (L.Result * 3)()
        fake = 4096
        rc = lib.lbfgs_batch_minimize_device(bt.h, L.OBJECTIVES["quad_sep"], 0, C.byref(k), fake, L.BATCH_PACKED, fake, 5,
                                             4, 1e-5, L.FLAG_QUIET, r3)
        assert rc == BAD_ARG and b"ragged" in lib.lbfgs_batch_last_error(bt.h)
        rc = lib.lbfgs_batch_minimize_device(bt.h, L.OBJECTIVES["quad_sep"], 0, C.byref(k), fake, 5, fake, L.BATCH_PACKED,
                                             4, 1e-5, L.FLAG_QUIET, r3)
        assert rc == BAD_ARG
        for strides in ((L.BATCH_PACKED, L.BATCH_PACKED, 5), (25, 5, L.BATCH_PACKED)):
            rc = lib.lbfgs_batch_set_dense_quadratics_device(bt.h, fake, strides[0], strides[1], fake, strides[2])
            assert rc == BAD_ARG and b"ragged" in lib.lbfgs_batch_last_error(bt.h)
        X5 = np.stack(x0s([5] * 3))
        res = bt.minimize("quad_sep", X5, "backtracking", max_iterations=4, trace=True)
        for p in range(3):
            check_problem(res, p, O.lbfgs("quad_sep", X5[p], "backtracking", m, 4, 1e-5, mode=O.CANON), "uniform after")
