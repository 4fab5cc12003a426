"""Line-search constant sets that are not the defaults — TEST INFRASTRUCTURE ONLY.

One table, imported by the fixture generator (tests/golden/make_consts.py), the oracle pin
(test_oracle_consts.py), the input conditions (test_constants_inputs.py) and the GPU parity
tests (test_gpu_constants.py: paths 1-10 and 13; devobj_gpu_cases.py: path 11, the device-callback
objective; batchcb_gpu_cases.py: path 12, the batched callback). The defaults (c1 1e-4, c2 0.9,
initial_step 1, backtracking_alpha 0.5, backtracking_tol 1e-8, wolfe_interp_min 1e-10) are powers
of two where it matters, which hides "multiply again" against "multiply the stored value" and 1.0
written for initial_step.

  K1  a ratio that is no power of two, strict c1: backtracking chains up to 0.7^19
  K2  a first step above 1 that is never accepted on the tridiagonal quadratic; Wolfe expands
  K3  a small first step, almost always accepted; backtracking-Wolfe grows it by 1.1 many times
  K4  a first step below the driver's 1e-10 floor (no backtracking-Wolfe: thousands of passes)
  K5  K1's ratio with a large tolerance and a large interpolation minimum: both are reached
"""
FIELDS = ("c1", "c2", "initial_step", "backtracking_alpha", "backtracking_tol", "wolfe_interp_min")

SETS = {
    "K1": dict(c1=0.3, c2=0.5, initial_step=1.0, backtracking_alpha=0.7, backtracking_tol=1e-6,
               wolfe_interp_min=1e-7),
    "K2": dict(c1=1e-3, c2=0.2, initial_step=2.5, backtracking_alpha=0.3, backtracking_tol=1e-8,
               wolfe_interp_min=1e-12),
    "K3": dict(c1=1e-4, c2=0.9, initial_step=0.01, backtracking_alpha=0.5, backtracking_tol=1e-8,
               wolfe_interp_min=1e-10),
    "K4": dict(c1=1e-4, c2=0.9, initial_step=5e-11, backtracking_alpha=0.5, backtracking_tol=1e-13,
               wolfe_interp_min=1e-14),
    "K5": dict(c1=0.3, c2=0.5, initial_step=1.0, backtracking_alpha=0.7, backtracking_tol=0.2,
               wolfe_interp_min=0.05),
}

SEARCHES = ("backtracking", "interpolation", "wolfe", "backtracking_wolfe")
SEED, LO, HI, TOL = 7, -2.0, 2.0, 1e-5


# ---- the inputs of tests/test_gpu_constants.py; tests/test_constants_inputs.py checks on the CPU
# ---- that the constants bite in every one of them ------------------------------------------------
# (set, objective, n, m, search, iterations). n = 1000: two segments of 512, the second masked;
# 4099 with m = 1: a one-pair history, nine segments; 70 001: segments of 2048; 257: one partly
# filled segment. Rosenbrock under K2 + Wolfe overflows after some 30 iterations, the separable
# quadratic under K1 / K5 + Wolfe at once, and the tridiagonal quadratic under K1 / K5 + Wolfe takes
# the default constants' steps: none of these is used.
SOLVES = [
    ("K1", "rosenbrock", 70_001, 5, "backtracking", 30),
    ("K1", "rosenbrock", 4099, 1, "backtracking", 30),
    ("K1", "rosenbrock", 1000, 5, "interpolation", 30),
    ("K1", "rosenbrock", 1000, 5, "wolfe", 30),            # fails at iteration 1, a negative step before
    ("K1", "rosenbrock", 4099, 1, "backtracking_wolfe", 30),
    ("K2", "quad_tridiag", 70_001, 5, "backtracking", 30),  # no first step accepted
    ("K2", "rosenbrock", 1000, 7, "backtracking", 30),
    ("K2", "quad_tridiag", 1000, 5, "interpolation", 30),
    ("K2", "quad_tridiag", 4099, 1, "wolfe", 25),           # expands above initial_step
    ("K2", "quad_tridiag", 70_001, 5, "backtracking_wolfe", 30),
    ("K5", "rosenbrock", 1000, 5, "backtracking", 30),      # ends on alpha < backtracking_tol
    ("K5", "rosenbrock", 1000, 5, "interpolation", 30),     # returns wolfe_interp_min
    ("K5", "rosenbrock", 257, 5, "wolfe", 30),
    ("K5", "rosenbrock", 70_001, 5, "backtracking_wolfe", 30),
    ("K3", "rosenbrock", 1000, 5, "backtracking_wolfe", 25),  # grows the step by 1.1 many times
    ("K4", "rosenbrock", 1000, 5, "backtracking", 30),      # initial_step < 1e-10: fails at once
    ("K4", "quad_tridiag", 4099, 1, "interpolation", 30),
    ("K4", "rosenbrock", 70_001, 5, "wolfe", 25),           # doubles its way up every iteration
]
BATCHED_TRIALS = SOLVES                                                       # path 1
SPECULATIVE = [c for c in SOLVES if c[0] in ("K1", "K2", "K3", "K4")]         # path 2
DEVICE_SEARCH = [c for c in SOLVES if c[0] != "K4"]                           # path 3

# path 4, vector-free (backtracking and interpolation only)
VECTOR_FREE = [(ks, obj, n, 5, ls, 25) for ks, obj in (("K1", "rosenbrock"), ("K2", "quad_tridiag"))
               for ls in ("backtracking", "interpolation") for n in (70_001, 1000)]
# paths 5 and 9, unfused and the CUDA-compat loops, n = 1000
UNFUSED = [(ks, obj, 1000, 5, ls, 25) for ks, obj in (("K1", "rosenbrock"), ("K2", "quad_tridiag")) for ls in SEARCHES]
CUDA_COMPAT = UNFUSED
# path 6, the external-objective loop: Rosenbrock as host callbacks, the dense quadratic mat100
HOST = [(ks, "rosenbrock", 1000, 5, ls, 20) for ks in ("K1", "K2", "K5") for ls in SEARCHES]
DENSE = [(ks, "dense", 100, 5, ls, 40) for ks in ("K1", "K2", "K5") for ls in SEARCHES]
# path 7, the batched solver, three problems (x0 seeds 1, 2, 3 / the fixture_batch recipe)
BATCH_STENCIL = [(ks, "quad_tridiag" if ks == "K2" else "rosenbrock", n, m, ls, 12)
                 for ks in ("K1", "K2", "K5") for ls in SEARCHES for n in (5, 513) for m in (1, 5)]
BATCH_DENSE = [(ks, "dense", n, 5, ls, 40) for ks in ("K1", "K2", "K5") for ls in SEARCHES for n in (10, 100)]
BATCH_SEEDS = (1, 2, 3)
BATCH_DENSE_Q = (0, 1, 3)  # (problem 2 of mat10 takes the default constants' steps under K1 / K5 + interpolation)
# the CUDA path's searches that read the file's own constants, not constants.h (L-BFGS.cu's cached
# backtracking-Wolfe; the variant files' backtracking and backtracking-Wolfe): (cuda, search)
CUDA_OWN_CONSTANTS = {(1, "backtracking_wolfe"), (2, "backtracking"), (2, "backtracking_wolfe")}
# path 8, lbfgs_line_search alone along -g from x0(seed LS_SEED) of Rosenbrock
LS_N, LS_SEED = 5000, 3
LINE_SEARCH = [(ks, ls) for ks in ("K1", "K2", "K5") for ls in SEARCHES]
# path 10, two emulated ranks, every rank owning segments
SHARDED = ("K2", "quad_tridiag", 2_100_001, 5, "wolfe", 10)
# path 11, the single-problem device-callback objective (LBFGS_OBJ_DEVICE), with and without
# eager_grad: the HOST list's shape, compared with the host-callback path too
DEVICE_OBJ = [(ks, "rosenbrock", 1000, 5, ls, 20) for ks in ("K1", "K2", "K5") for ls in SEARCHES]
# path 12, the batched callback (k_batch_solve_ext: a search is an lbk_search record stored between
# launches and resumed), four problems from batch_x0. K1 / K5 + Wolfe on Rosenbrock fail their
# search at iteration 1 for three of the four starts and the fourth runs on; K2 + Wolfe on the
# tridiagonal quadratic expands every iteration.
BATCH_CALLBACK = [(ks, "quad_tridiag" if ks == "K2" else "rosenbrock", n, m, ls, 12)
                  for ks in ("K1", "K2", "K5") for ls in SEARCHES for n in (5, 513) for m in (1, 5)]
BATCH_CALLBACK += [
    ("K3", "rosenbrock", 513, 5, "backtracking_wolfe", 12),  # grows the step by 1.1 some 24 times per search
    ("K3", "quad_tridiag", 513, 5, "backtracking", 12),
    ("K3", "rosenbrock", 513, 5, "wolfe", 12),               # problems that end inside their first search
    ("K4", "rosenbrock", 513, 5, "backtracking", 12),        # initial_step < 1e-10: fails at once
]
# the resumable record alone: backtracking_alpha = 0.99 (tests/test_gpu_device_search.py's constant).
# One row rejects hundreds of steps in its first search, a round each, beside two rows that start
# within 1e-10 of Rosenbrock's minimiser and are done after their first evaluation.
LONG_SEARCH = dict(objective="rosenbrock", n=513, m=3, search="backtracking", iterations=2, row=1,
                   consts=dict(backtracking_alpha=0.99), rejected_at_least=300)
# path 13, ragged batches. Stencil: sizes [513, 5, 1537, 129], problem p from x0 seed 1 + p; dense:
# sizes [10, 100, 10] of the known-answer data, problems q = 0, 1, 3 of the dense_problem recipe
RAGGED_SIZES = (513, 5, 1537, 129)
RAGGED_DENSE_SIZES, RAGGED_DENSE_Q = (10, 100, 10), (0, 1, 3)
BATCH_RAGGED = [(ks, "quad_tridiag" if ks == "K2" else "rosenbrock", RAGGED_SIZES, m, ls, 12)
                for ks in ("K1", "K2", "K5") for ls in SEARCHES for m in (1, 5)]
BATCH_RAGGED_DENSE = [(ks, "dense", RAGGED_DENSE_SIZES, m, ls, 40)
                      for ks in ("K1", "K2", "K5") for ls in SEARCHES for m in (1, 5)]


def batch_x0(n):
    """the four starts of the batched callback's tests (hist_cases.x0_batch): two in [-2, 2], one of
    those scaled by 1e-3, one within 1e-4 of the all-ones point"""
    import hist_cases

    return hist_cases.x0_batch(n)


def long_search_x0():
    import numpy as np

    import oracle_lib as O

    n = LONG_SEARCH["n"]
    X0 = np.stack([O.x0_uniform(n, 5, 1.0 - 1e-10, 1.0 + 1e-10), O.x0_uniform(n, 17, LO, HI),
                   O.x0_uniform(n, 6, 1.0 - 1e-10, 1.0 + 1e-10)])
    return X0


def ragged_id(case):
    return "-".join("x".join(str(n) for n in v) if isinstance(v, tuple) else str(v) for v in case)


def ragged_problems(case):
    """the problems of a BATCH_RAGGED or BATCH_RAGGED_DENSE case, each as a uniform case of its own
    size with the keyword arguments of oracle() that select it"""
    ks, obj, sizes, m, ls, iters = case
    if obj == "dense":
        return [((ks, obj, n, m, ls, iters), dict(seed=10 + q, dense_q=q)) for n, q in zip(sizes, RAGGED_DENSE_Q)]
    return [((ks, obj, n, m, ls, iters), dict(seed=1 + p)) for p, n in enumerate(sizes)]


_runs = {}


def dense_problem(n, q=0):
    """(A, b) of the known-answer data of size n, as problem q of test_gpu_batch_dense.py's
    fixture_batch recipe: A + 0.25 q I, (1 + q) b (its x0 comes from seed 10 + q)."""
    import os

    import numpy as np

    import oracle_lib as O

    if "data" not in _runs:
        _runs["data"] = np.load(os.path.join(O.GOLDEN, "matrices.npz"), allow_pickle=False)
    d = _runs["data"]
    return (d[f"mat{n}"] + 0.25 * q * np.eye(n), (1.0 + q) * d[f"linear{n}"])


def oracle(case, seed=SEED, default=False, vector_free=False, cuda=0, host=False, dense_q=None, x0=None, maxit=None):
    """The canonical-order oracle's run of a case with its set's constants (default=True: with the
    default constants), computed once per argument list, shared and left unchanged.
    host: the objective through Python callables; dense_q: problem q of the dense data."""
    import numpy as np

    import oracle_lib as O

    ks, obj, n, m, ls, iters = case
    key = (case, seed, default, vector_free, cuda, host, dense_q, maxit, None if x0 is None else x0.tobytes())
    if key not in _runs:
        if x0 is None:
            x0 = O.x0_uniform(n, seed, LO, HI)
        consts = None if default else SETS[ks]
        kw = dict(mode=O.CANON, consts=consts, vector_free=vector_free, cuda=cuda)
        if cuda and default:
            kw["consts"] = O.CONSTANTS_H
        if obj == "dense":
            O.dense_set(*dense_problem(n, dense_q or 0))
        with np.errstate(all="ignore"):
            if host:
                r = O.lbfgs("host", x0, ls, m, maxit or iters, TOL, f=lambda x: O.f(obj, x, O.CANON),
                            grad=lambda x: O.grad(obj, x), **kw)
            else:
                r = O.lbfgs(obj, x0, ls, m, maxit or iters, TOL, log_calls=True, **kw)
        r["x0"] = x0
        _runs[key] = r
    return _runs[key]


def device_constants(L, name):
    """lbfgs_constants of a set (wolfe_interp_max stays the default: no search reads it)."""
    k = L.constants()
    for f in FIELDS:
        setattr(k, f, SETS[name][f])
    return k
