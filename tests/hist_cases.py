"""Inputs that fill and rotate a long history in the batched solver — TEST INFRASTRUCTURE ONLY.

lbfgs_batch_create* accept 1 <= m <= 16 (LBK_SMALL_HMAX): BatchState::ring[16], sy[17], yy[17],
BatchWave::TA[16], LBK_BATCH_NVEC(m) = 7 + 2 (m + 1) and the spare-pair rotation of batch_accept
are sized for that. One table of batches with m = 16 and m = 8, imported by the input conditions
(tests/test_history_inputs.py, CPU, the oracle alone) and by the GPU tests of the five batch kernel
families (test_gpu_batch.py, test_gpu_batch_ragged.py, test_gpu_batch_dense.py,
batchcb_gpu_cases.py), which compare bits with the canonical-order oracle and the single-problem
path. The oracle runs are computed once per case, shared and left unchanged.

  STENCIL         B = 4, the starts of x0_batch: Rosenbrock, m = 16, tolerance 1e-7, 40 iterations
                  at most, n = 5 (a history longer than the problem is wide), 17, 513, 1537; the
                  tridiagonal quadratic (12 iterations at most from these starts: it cannot fill 16
                  pairs), m = 8, tolerance 1e-9, n = 513. Run by the uniform stencil batch and by
                  the callback batch.
  RAGGED_STENCIL  sizes [1537, 17, 513] in one batch, the same two objectives.
  DENSE           n = 65 and 513, m = 16, three problems: two with the eigenvalues 1 ... 1000 (40
                  iterations), one with 1 ... 10, which converges earlier.
  RAGGED_DENSE    sizes [513, 65, 100], m = 16, the same spectra.
"""
import numpy as np

import oracle_lib as O

SEARCHES = ("backtracking", "interpolation", "wolfe", "backtracking_wolfe")
MAXIT = 40


def x0_batch(n):
    """Four starts: two in [-2, 2], one of those scaled by 1e-3, and one within 1e-4 of the all-ones
    point, Rosenbrock's minimiser, so that the problems of a batch end at different iterations."""
    return np.stack([O.x0_uniform(n, 1, -2.0, 2.0), 1e-3 * O.x0_uniform(n, 2, -2.0, 2.0),
                     O.x0_uniform(n, 3, 1.0 - 1e-4, 1.0 + 1e-4), O.x0_uniform(n, 4, -2.0, 2.0)])


# (objective, n, m, search, tolerance, the problems end at different iterations)
# Under the Wolfe search at n = 513 and 1537 all four Rosenbrock starts run into the limit of 40.
STENCIL = [("rosenbrock", n, 16, ls, 1e-7, not (ls == "wolfe" and n >= 513))
           for n in (5, 17, 513, 1537) for ls in SEARCHES]
STENCIL += [("quad_tridiag", 513, 8, ls, 1e-9, True) for ls in SEARCHES]

# (objective, sizes, the start of x0_batch each problem takes, m, search, tolerance, differ)
RAGGED_SIZES = [1537, 17, 513]
RAGGED_STENCIL = [("rosenbrock", RAGGED_SIZES, (0, 2, 3), 16, ls, 1e-7, True) for ls in SEARCHES]
RAGGED_STENCIL += [("quad_tridiag", RAGGED_SIZES, (3, 1, 0), 8, ls, 1e-9, True) for ls in SEARCHES]

# (n, m, search): problems 0 and 1 with the eigenvalues 1 ... 1000, problem 2 with 1 ... 10
DENSE_M, DENSE_TOL = 16, 1e-5
DENSE = [(n, DENSE_M, ls) for n in (65, 513) for ls in SEARCHES]
RAGGED_DENSE_SIZES = [513, 65, 100]
RAGGED_DENSE = [(tuple(RAGGED_DENSE_SIZES), DENSE_M, ls) for ls in SEARCHES]


def case_id(c):
    return "-".join("x".join(str(n) for n in v) if isinstance(v, (list, tuple)) else str(v) for v in c)


def stencil_x0(case):
    return x0_batch(case[1])


def ragged_x0(case):
    return [x0_batch(n)[k] for n, k in zip(case[1], case[2])]


def spectrum_problem(n, eig, seed):
    """(A, b, x0) as test_gpu_batch_dense.py's spectrum_batch makes one problem: A with the
    eigenvalues `eig` in a random orthogonal basis, symmetrised; b and x0 random."""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    M = (Q * eig) @ Q.T
    return (M + M.T) / 2, rs.uniform(-1.0, 1.0, n), O.x0_uniform(n, seed, -2.0, 2.0)


_data = {}


def dense_data(n):
    """Three problems of size n: (A (3, n, n), b (3, n), X0 (3, n))"""
    if n not in _data:
        wide, narrow = np.logspace(0, 3, n), np.logspace(0, 1, n)
        _data[n] = tuple(np.stack(v) for v in zip(*[spectrum_problem(n, eig, 4000 + n + p)
                                                     for p, eig in enumerate((wide, wide, narrow))]))
    return _data[n]


def ragged_dense_data():
    """Problem p of size RAGGED_DENSE_SIZES[p]: lists A, b, X0; the smallest has the narrow spectrum"""
    if "ragged" not in _data:
        A, b, X0 = [], [], []
        for p, n in enumerate(RAGGED_DENSE_SIZES):
            a, v, x = spectrum_problem(n, np.logspace(0, 1 if n == min(RAGGED_DENSE_SIZES) else 3, n), 5000 + n)
            A.append(a), b.append(v), X0.append(x)
        _data["ragged"] = (A, b, X0)
    return _data["ragged"]


class Callables:
    """an objective of the oracle as the Python callables f and grad"""

    def __init__(self, obj):
        self.obj = obj

    def f(self, x):
        return O.f(self.obj, x, O.CANON)

    def grad(self, x):
        return O.grad(self.obj, x)


_runs = {}


def _shared(key, make):
    if key not in _runs:
        with np.errstate(all="ignore"):
            _runs[key] = make()
    return _runs[key]


def stencil_oracle(case, host=None):
    """The oracle's runs of a STENCIL or RAGGED_STENCIL batch. host: a factory of an object with the
    objective as the callables f and grad (the callback batch's reference), one per problem."""
    obj, m, ls, tol = case[0], case[-4], case[-3], case[-2]
    X0 = ragged_x0(case) if isinstance(case[1], (list, tuple)) else stencil_x0(case)

    def make():
        if host is None:
            return [O.lbfgs(obj, x0, ls, m, MAXIT, tol, mode=O.CANON) for x0 in X0]
        runs = []
        for x0 in X0:
            cb = host(obj)
            runs.append(O.lbfgs("host", x0, ls, m, MAXIT, tol, mode=O.CANON, f=cb.f, grad=cb.grad))
        return runs

    return _shared((case_id(case), host is not None), make)


def dense_oracle(case):
    """The oracle's runs of a DENSE or RAGGED_DENSE batch"""
    n, m, ls = case
    A, b, X0 = ragged_dense_data() if isinstance(n, tuple) else dense_data(n)

    def make():
        runs = []
        for p in range(len(X0)):
            O.dense_set(A[p], b[p])
            runs.append(O.lbfgs("dense", X0[p], ls, m, MAXIT, DENSE_TOL, mode=O.CANON))
        return runs

    return _shared(("dense", case_id(case)), make)


MESSAGES = ["Not a descent direction", "Skipping update", "Invalid rho", "Invalid gamma", "Line search failed"]
EVENT_KEYS = ["not_descent", "skipped_updates", "invalid_rho", "invalid_gamma"]
COUNTS = ("iterations", "trials_f", "trials_fg", "commits", "h_min", "h_max")


def same_bits(a, b):
    """equal bit for bit, a NaN (the trace's "no step" mark) equal to a NaN in the same place"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def check_single(res, p, one, what):
    """Problem p of a batch result against a traced run of the single-problem path (Context.minimize):
    x, f, |g|, status, iterations, trials_f, trials_fg, commits, h_min, h_max, the four event counts
    (the single path's messages counted) and the trace."""
    assert same_bits(res["x"][p], one["x"]), (what, p)
    assert same_bits([res["f"][p], res["gnorm"][p]], [one["f"], one["gnorm"]]), (what, p)
    assert res["status"][p] == one["status"], (what, p, res["status"][p], one["status"])
    for key in COUNTS:
        assert res[key][p] == one[key], (what, p, key, res[key][p], one[key])
    for key in ("tr_f", "tr_gnorm", "tr_alpha"):
        assert same_bits(res[key][p], one[key]), (what, p, key)
    want = [sum(1 for line in one["messages"].splitlines() if m in line) for m in MESSAGES]
    assert [res["events"][p][k] for k in EVENT_KEYS] == want[:4], (what, p, res["events"][p], want)


def check_h_max(res, orc, m, what):
    """h_max == m for the problems the CPU condition says fill the ring, at least two of the batch"""
    full = [p for p, o in enumerate(orc) if full_ring(o, m)]
    assert len(full) >= 2, (what, full)
    for p in full:
        assert res["h_max"][p] == m and res["h_min"][p] == 0, (what, p, res["h_min"][p], res["h_max"][p])


def skipped_updates(o):
    """Pairs the standard path did not store: its "Skipping update" lines. (The oracle's "skips" field
    counts something else, the first-loop pairs the CUDA path's loop passes over, and stays 0 here.)"""
    return sum(1 for line in o["messages"].splitlines() if "Skipping update" in line)


def full_ring(o, m):
    """the run stored m pairs and went on for four more accepted updates: h reaches m and the ring,
    with its spare pair, rotates"""
    return o["iters"] - skipped_updates(o) >= m + 4


# Skipped updates of the four starts of x0_batch, for the STENCIL cases that have any (every other case
# has none); the builtin objective and the callables give the same. At n = 5 the start scaled by 1e-3
# skips 19 of its 40 updates under the two searches without a curvature condition. full_ring still holds
# for it, 40 - 19 = 21 >= 16 + 4, so three of the four problems fill and rotate the ring as before (the
# fourth, the start at the minimiser, converges after 19 iterations).
STENCIL_SKIPS = {("rosenbrock", 5, 16, ls): [0, 19, 0, 0] for ls in ("backtracking", "interpolation")}


def stencil_skips(case):
    return STENCIL_SKIPS.get(tuple(case[:4]), [0, 0, 0, 0])


# ---- histories of 17 to 64 pairs on the single-problem paths ----
# h = 17 is where a small-n solve leaves the one-launch cooperative iteration (LBK_SMALL_HMAX = 16) for
# the launch sequence, in mid-solve; m = 64 is the driver's limit (MMAX). Rosenbrock from
# x0_uniform(n, 1, -2, 2), tolerance 1e-7: every run ends at its iteration limit, fills the ring and
# rotates it through at least 12 further stored pairs (tests/test_history_inputs.py).
LONG_TOL, LONG_SEED = 1e-7, 1
LONG_M = ((17, 30), (24, 40), (64, 80))  # (m, iteration limit)
LONG_N = (17, 513, 1537)                 # one segment, two, and four
# (n, m, search, iteration limit)
SINGLE_LONG = [(n, m, ls, it) for n in LONG_N for m, it in LONG_M for ls in SEARCHES]
# larger n: 196 segments (the cooperative forms' range) and 342 segments of 2048 (deferred stage 2)
SINGLE_LONG_LARGE = [(n, 64, ls, 80) for n in (4097, 100_003) for ls in SEARCHES] + [(700_001, 24, "wolfe", 30)]
# the cases whose oracle run prints "Skipping update", and how often; every other case: never
LONG_SKIPS = {(1537, 64, "backtracking", 80): 1, (1537, 64, "interpolation", 80): 1}


# the SINGLE_LONG cases that continue a line search on the device (k_coop_search) at an iteration with 17
# pairs or more, after a two-loop run as the launch sequence; every other case does not
# (tests/test_gpu_long_history.py::test_device_search_beyond_16_pairs asserts exactly this list)
# With seed 1 every line search has such a case, so no other seed was needed. Plain backtracking has two:
# its first rejected step is usually settled by the candidate the commit evaluates in the same pass.
_NO_DEVICE_SEARCH = {(n, m, "backtracking", it) for n in LONG_N for m, it in LONG_M if (n, m) not in ((1537, 24), (1537, 64))}
_NO_DEVICE_SEARCH |= {(513, 24, "interpolation", 40), (513, 24, "backtracking_wolfe", 40), (1537, 17, "wolfe", 30)}
LONG_DEVICE_SEARCH = [c for c in SINGLE_LONG if c not in _NO_DEVICE_SEARCH]


def long_id(c):
    return f"n{c[0]}-m{c[1]}-{c[2]}-it{c[3]}"


def long_x0(n):
    return O.x0_uniform(n, LONG_SEED, -2.0, 2.0)


def long_oracle(case):
    """the oracle's canonical-order run of a SINGLE_LONG / SINGLE_LONG_LARGE case: computed once, shared
    by the tests that need it and left unchanged"""
    n, m, ls, it = case
    return _shared(("long", case), lambda: O.lbfgs("rosenbrock", long_x0(n), ls, m, it, LONG_TOL, mode=O.CANON))


def long_cuda_oracle(ls, cuda):
    """the oracle's restatement of the CUDA path's loop (cuda = 1) or of its variant files' (2) at n = 513,
    m = 64, 80 iterations, constants.h's constants: the ring slot k % m wraps at k = 64"""
    return _shared(("long_cuda", ls, cuda), lambda: O.lbfgs("rosenbrock", long_x0(513), ls, 64, 80, LONG_TOL, mode=O.CANON,
                                                            cuda=cuda, consts=dict(c2=0.7)))


def late_searches(o, k0=18):
    """iterations k >= k0 whose accepted step is not the initial step: a line search that went past its
    first trial while more than 16 pairs were stored"""
    a = o["alpha"][:o["iters"]]
    return [k for k in range(k0, len(a)) if a[k] != 1.0]


# ---- the two-loop primitive ----
def twoloop_inputs(h, n):
    """g and h pairs with s.y > 0, as test_gpu_parity.py's test_twoloop_bit_exact draws them"""
    rs = np.random.RandomState(100 * h + n)
    g = rs.uniform(-1, 1, n)
    S = [rs.uniform(-1, 1, n) for _ in range(h)]
    Y = [s * rs.uniform(0.5, 2.0, n) + 0.01 * rs.uniform(-1, 1, n) for s in S]  # s.y > 0
    return g, S, Y


TWOLOOP_LONG = [(h, n) for h in (17, 64) for n in (3, 1000, 70_001)]
# ||d - d_ref|| <= TWOLOOP_BOUND ||d_ref|| against the long-double recursion. The oracle's own difference
# on the six TWOLOOP_LONG inputs lies between 6.1e-17 and 5.5e-16 (CPU); the bound is 18 times the
# largest of them and is asserted for the oracle alone in tests/test_history_inputs.py.
TWOLOOP_BOUND = 1e-14


def twoloop_longdouble(g, S, Y):
    """The two-loop recursion (lbfgs.cpp:94-143) in numpy.longdouble, every sum left to right."""
    ld = np.longdouble

    def dot(a, b):
        return np.cumsum(a * b)[-1]

    g = g.astype(ld)
    S, Y = [s.astype(ld) for s in S], [y.astype(ld) for y in Y]
    h = len(S)
    q, al = g.copy(), [None] * h
    for i in range(h - 1, -1, -1):
        al[i] = dot(S[i], q) / dot(Y[i], S[i])
        q = q - al[i] * Y[i]
    r = q * (dot(S[h - 1], Y[h - 1]) / dot(Y[h - 1], Y[h - 1]))
    for i in range(h):
        beta = dot(Y[i], r) / dot(Y[i], S[i])
        r = r + S[i] * (al[i] - beta)
    return -r


def twoloop_error(d, dref):
    """||d - d_ref|| / ||d_ref||, formed in long double"""
    e = np.asarray(d, np.longdouble) - dref
    return float(np.sqrt(np.sum(e * e)) / np.sqrt(np.sum(dref * dref)))

