"""GPU parity with the line-search constants varied (lbfgs_constants: c1, c2, initial_step,
backtracking_alpha, backtracking_tol, wolfe_interp_min), on every path that restates them.

The constant sets and the cases are tests/consts_cases.py's; tests/test_constants_inputs.py asserts
on the CPU that the constants bite in each case; tests/test_oracle_consts.py pins the oracle with
these constants to the reference's own code. Here every path is compared, bit for bit, with the
canonical-order oracle run with the same constants (the f / |g| / step traces, the x checksums, the
final x, status, iteration count and messages) and, where it has an off-switch, with the
switched-off run (the same bits and counters). Each case asserts that its path ran. Paths 11 (the
device-callback objective) and 12 (the batched callback) need torch in the process and are in
tests/devobj_gpu_cases.py and tests/batchcb_gpu_cases.py; path 13, ragged batches, is here.
"""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import consts_cases as K  # noqa: E402
import lbfgs_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("LBFGS_COOP", "LBFGS_BATCH", "LBFGS_SPEC", "LBFGS_DEV_SEARCH", "LBFGS_DEV_WOLFE", "LBFGS_SEARCH_TIMEOUT",
         "LBFGS_DIRECT", "LBFGS_TICKET")
MESSAGES = ["Not a descent direction", "Skipping update", "Invalid rho", "Invalid gamma", "Line search failed"]
EVENT_KEYS = ["not_descent", "skipped_updates", "invalid_rho", "invalid_gamma"]


def _id(c):
    return "-".join(str(v) for v in c)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    """equal bit for bit, a NaN (the trace's "no step" mark) equal to a NaN in the same place"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def solve(monkeypatch, case, env=(), **kw):
    """one solve of a case with its set's constants in a fresh context (the knobs are read at creation)"""
    ks, obj, n, m, ls, iters = case
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)
    x0 = K.oracle(case)["x0"] if "x0" not in kw else kw.pop("x0")
    with L.Context(n, m) as c:
        r = c.minimize(obj, x0, ls, iters, tolerance=K.TOL, trace=True, consts=K.device_constants(L, ks), **kw)
        r["spec"], r["search"] = c.spec_stats(), c.search_stats()
    return r


def check_oracle(r, o, what):
    """the compared fields of a single-problem run against its oracle run"""
    assert len(r["tr_f"]) == len(o["f"]), what
    assert np.array_equal(bits(r["tr_f"]), bits(o["f"])), what
    assert np.array_equal(bits(r["tr_gnorm"]), bits(o["gnorm"])), what
    assert same_bits(r["tr_alpha"], o["alpha"]), (what, r["tr_alpha"], o["alpha"])
    assert np.array_equal(r["tr_c1"], o["c1"]) and np.array_equal(r["tr_c2"], o["c2"]), what
    assert np.array_equal(bits(r["x"]), bits(o["x"])), what
    assert r["status"] == o["status"] and r["iterations"] == o["iters"], (what, r["status"], r["iterations"])
    assert r["messages"] == o["messages"], what


def check_same(a, b, what, counters=True):
    for key in ("tr_f", "tr_gnorm", "x"):
        assert np.array_equal(bits(a[key]), bits(b[key])), (what, key)
    assert same_bits(a["tr_alpha"], b["tr_alpha"]), what
    assert np.array_equal(a["tr_c1"], b["tr_c1"]) and np.array_equal(a["tr_c2"], b["tr_c2"]), what
    assert a["messages"] == b["messages"] and a["status"] == b["status"] and a["iterations"] == b["iterations"], what
    assert bits([a["f"], a["gnorm"]]).tolist() == bits([b["f"], b["gnorm"]]).tolist(), what
    if counters:
        for k in ("trials_f", "trials_fg", "commits"):
            assert a[k] == b[k], (what, k, a[k], b[k])


# ---- 1. the launch sequence with batched trials ---------------------------------------------------
@pytest.mark.parametrize("case", K.BATCHED_TRIALS, ids=_id)
def test_batched_trials(monkeypatch, case):
    """the halving chains formed by repeated multiplication, the first commit's candidate a0 * beta.

    Under K2 the Wolfe search rejects all of its 19 trial steps per iteration on f alone, a pass
    each. Reading d formed on the fly for an iteration's first two trial passes and materialising it
    for the third costs 2 P + 6 vectors for P >= 3 passes against 2 P + 4 with d materialised first:
    this case moved 48 925 664 bytes against 47 450 024 without batching (n = 4099, m = 1, 25
    iterations) until the driver learnt from the last search's pass count to materialise d first."""
    one = solve(monkeypatch, case, {"LBFGS_COOP": "0", "LBFGS_BATCH": "0"})
    bat = solve(monkeypatch, case, {"LBFGS_COOP": "0", "LBFGS_BATCH": "1"})
    print(f"{_id(case)}: passes {one['passes']} -> {bat['passes']}, bytes {one['bytes']:.0f} -> {bat['bytes']:.0f}, "
          f"trials f/fg {one['trials_f']}/{one['trials_fg']} -> {bat['trials_f']}/{bat['trials_fg']}")
    check_oracle(bat, K.oracle(case), case)
    check_same(one, bat, case, counters=False)  # (a batched pass counts once for several steps)
    assert bat["spec"] == (0, 0) and bat["search"] == (0, 0)  # no cooperative launch
    assert bat["passes"] <= one["passes"], (bat["passes"], one["passes"])
    assert bat["bytes"] <= one["bytes"], (bat["bytes"], one["bytes"])
    ks, obj, n, m, ls, iters = case
    if ks != "K4" or ls == "wolfe":  # (K4's other searches fail before any trial pass)
        assert one["trials_f"] + one["trials_fg"] > 0
    if ls in ("backtracking", "interpolation") and ks != "K4":
        assert one["trials_f"] > 0
    if (ks, obj, ls) == ("K2", "quad_tridiag", "backtracking"):
        assert bat["commits"] > bat["iterations"]  # every iteration recommits


# ---- 2. the cooperative iteration with the speculative next launch --------------------------------
@pytest.mark.parametrize("case", K.SPECULATIVE, ids=_id)
def test_speculative(monkeypatch, case):
    """the prologue's c1, c2 and a0, and the host's gate on initial_step before a launch is queued"""
    off = solve(monkeypatch, case, {"LBFGS_SPEC": "0"})
    on = solve(monkeypatch, case, {"LBFGS_SPEC": "1"})
    check_oracle(on, K.oracle(case), case)
    check_same(off, on, case)
    assert off["spec"] == (0, 0)
    adopted, dropped = on["spec"]
    ks, obj, n, m, ls, iters = case
    assert adopted <= on["iterations"]
    if ks == "K4":
        assert (adopted, dropped) == (0, 0)  # nothing is queued below 1e-10
    elif ks == "K3" or (ks == "K1" and ls != "wolfe"):
        assert adopted > 0, on["spec"]
    elif ks == "K2" and obj == "quad_tridiag":
        # no first step is accepted: no launch queued behind an iteration's first commit is taken
        assert dropped > 0, on["spec"]


# ---- 3. the device-resident searches --------------------------------------------------------------
@pytest.mark.parametrize("case", K.DEVICE_SEARCH, ids=_id)
def test_device_search(monkeypatch, case):
    """k_coop_search's init, beta, tol and amin"""
    host = solve(monkeypatch, case, {"LBFGS_DEV_SEARCH": "0"})
    dev = solve(monkeypatch, case, {"LBFGS_DEV_SEARCH": "1"})
    check_oracle(dev, K.oracle(case), case)
    check_same(host, dev, case)
    assert host["search"] == (0, 0)
    launches, commits = dev["search"]
    assert launches > 0 and commits <= launches, dev["search"]
    assert 0 <= dev["passes"] - host["passes"] <= launches, (host["passes"], dev["passes"], launches)


# ---- 4. vector-free -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.VECTOR_FREE, ids=_id)
def test_vector_free(monkeypatch, case):
    r = solve(monkeypatch, case, vector_free=True)
    check_oracle(r, K.oracle(case, vector_free=True), case)
    assert r["commits"] > 0


# ---- 5. unfused -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.UNFUSED, ids=_id)
def test_unfused(monkeypatch, case):
    r = solve(monkeypatch, case, unfused=True)
    check_oracle(r, K.oracle(case), case)
    assert r["spec"] == (0, 0) and r["search"] == (0, 0)  # neither fused launch form ran


# ---- 6. the external-objective loop ---------------------------------------------------------------
@pytest.mark.parametrize("case", K.HOST, ids=_id)
def test_host_callbacks(monkeypatch, case):
    ks, obj, n, m, ls, iters = case
    o = K.oracle(case, host=True)
    hc = (ks, "host", n, m, ls, iters)
    r = solve(monkeypatch, hc, x0=o["x0"], f=lambda x: O.f(obj, x, O.CANON), grad=lambda x: O.grad(obj, x))
    check_oracle(r, o, case)
    assert r["f_calls"] > 0 and r["grad_calls"] > 0


@pytest.mark.parametrize("case", K.DENSE, ids=_id)
def test_dense_quadratic(monkeypatch, case):
    ks, obj, n, m, ls, iters = case
    o = K.oracle(case)
    A, b = K.dense_problem(n)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    with L.Context(n, m) as c:
        c.set_dense_quadratic(A, b)
        r = c.minimize("dense", o["x0"], ls, iters, tolerance=K.TOL, trace=True, consts=K.device_constants(L, ks))
    check_oracle(r, o, case)


# ---- 7. the batched solver ------------------------------------------------------------------------
def check_problem(res, p, o, what):
    assert res["status"][p] == o["status"] and res["iterations"][p] == o["iters"], (what, p)
    assert same_bits(res["x"][p], o["x"]), (what, p)
    assert same_bits([res["gnorm"][p]], [o["gnorm"][-1]]), (what, p)
    if o["status"] != "ls_failed":  # (f at a failed step is not in the oracle's trace)
        assert same_bits([res["f"][p]], [o["f"][-1]]), (what, p)
    assert len(res["tr_f"][p]) == len(o["f"]), (what, p)
    assert same_bits(res["tr_f"][p], o["f"]) and same_bits(res["tr_gnorm"][p], o["gnorm"]), (what, p)
    assert same_bits(res["tr_alpha"][p], o["alpha"]), (what, p)
    want = [sum(1 for line in o["messages"].splitlines() if m in line) for m in MESSAGES]
    assert [res["events"][p][k] for k in EVENT_KEYS] == want[:4], (what, p, res["events"][p], want)
    assert (res["status"][p] == "ls_failed") == (want[4] > 0), (what, p)


def check_single(res, p, one, what):
    assert same_bits(res["x"][p], one["x"]), (what, p)
    assert same_bits([res["f"][p], res["gnorm"][p]], [one["f"], one["gnorm"]]), (what, p)
    assert res["iterations"][p] == one["iterations"] and res["status"][p] == one["status"], (what, p)
    for k in ("trials_f", "trials_fg", "commits"):
        assert res[k][p] == one[k], (what, p, k, res[k][p], one[k])


@pytest.mark.parametrize("case", K.BATCH_STENCIL, ids=_id)
def test_batch_stencil(case):
    """BatchIter's copy of the constants (a.K.*) in the stencil kernel"""
    ks, obj, n, m, ls, iters = case
    orc = [K.oracle(case, seed=s) for s in K.BATCH_SEEDS]
    X0 = np.stack([o["x0"] for o in orc])
    k = K.device_constants(L, ks)
    with L.Batch(n, m, len(X0)) as b:
        res = b.minimize(obj, X0, ls, max_iterations=iters, tolerance=K.TOL, consts=k, trace=True)
    assert res["launches"] > 0
    for p, o in enumerate(orc):
        check_problem(res, p, o, case)
    if (ks, n, m) == ("K1", 513, 5):  # one batch per search against the single-problem path
        with L.Context(n, m) as c:
            for p in range(len(X0)):
                check_single(res, p, c.minimize(obj, X0[p], ls, iters, tolerance=K.TOL, consts=k), case)


@pytest.mark.parametrize("case", K.BATCH_DENSE, ids=_id)
def test_batch_dense(case):
    """the same in the dense kernel, each problem with its own A and b"""
    ks, obj, n, m, ls, iters = case
    orc = [K.oracle(case, seed=10 + q, dense_q=q) for q in K.BATCH_DENSE_Q]
    X0 = np.stack([o["x0"] for o in orc])
    A = np.stack([K.dense_problem(n, q)[0] for q in K.BATCH_DENSE_Q])
    bb = np.stack([K.dense_problem(n, q)[1] for q in K.BATCH_DENSE_Q])
    k = K.device_constants(L, ks)
    with L.Batch(n, m, len(X0)) as b:
        b.set_dense_quadratics(A, bb)
        res = b.minimize("dense", X0, ls, max_iterations=iters, tolerance=K.TOL, consts=k, trace=True)
    assert res["launches"] > 0
    for p, o in enumerate(orc):
        check_problem(res, p, o, case)
    if (ks, n) == ("K2", 10):
        with L.Context(n, m) as c:
            for p in range(len(X0)):
                c.set_dense_quadratic(A[p], bb[p])
                check_single(res, p, c.minimize("dense", X0[p], ls, iters, tolerance=K.TOL, consts=k), case)


# ---- 13. ragged batches ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.BATCH_RAGGED + K.BATCH_RAGGED_DENSE, ids=K.ragged_id)
def test_batch_ragged(case):
    """the same constants in the ragged stencil and dense kernels: problems of different sizes in one
    batch, each against the oracle and against a single-problem solve of its own, counters included"""
    ks, obj, sizes, m, ls, iters = case
    subs = K.ragged_problems(case)
    orc = [K.oracle(sub, **kw) for sub, kw in subs]
    X0 = [o["x0"] for o in orc]
    k = K.device_constants(L, ks)
    data = [K.dense_problem(sub[2], kw["dense_q"]) for sub, kw in subs] if obj == "dense" else None
    with L.Batch(list(sizes), m) as b:
        assert b.ragged
        if data:
            b.set_dense_quadratics([d[0] for d in data], [d[1] for d in data])
        res = b.minimize(obj, X0, ls, max_iterations=iters, tolerance=K.TOL, consts=k, trace=True)
    assert res["launches"] > 0
    for p, o in enumerate(orc):
        check_problem(res, p, o, case)
        with L.Context(sizes[p], m) as c:
            if data:
                c.set_dense_quadratic(*data[p])
            check_single(res, p, c.minimize(obj, X0[p], ls, iters, tolerance=K.TOL, consts=k), case)


# ---- 8. lbfgs_line_search alone -------------------------------------------------------------------
@pytest.mark.parametrize("ks,ls", K.LINE_SEARCH)
def test_line_search_alone(monkeypatch, ks, ls):
    """along -g from a random Rosenbrock point: the step of iteration 0 of an oracle run from there,
    whichever form runs it"""
    n = K.LS_N
    o = K.oracle((ks, "rosenbrock", n, 2, ls, 1), seed=K.LS_SEED)
    x = o["x0"]
    g = O.grad("rosenbrock", x)
    got = {}
    for name, env in (("default", {}), ("one_pass_per_step", {"LBFGS_BATCH": "0"}), ("host_loop", {"LBFGS_DEV_SEARCH": "0"})):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with L.Context(n, 2) as c:
            got[name] = c.line_search("rosenbrock", ls, x, -g, g, consts=K.device_constants(L, ks))
    assert bits([got["default"]])[0] == bits([o["alpha"][0]])[0], (got, o["alpha"][0])
    assert bits([got["one_pass_per_step"]])[0] == bits([got["default"]])[0], got
    assert bits([got["host_loop"]])[0] == bits([got["default"]])[0], got


# ---- 9. the CUDA-compat loops with constants that are not the CUDA profile ------------------------
@pytest.mark.parametrize("variant", [False, True], ids=["loop", "variant"])
@pytest.mark.parametrize("case", K.CUDA_COMPAT, ids=_id)
def test_cuda_compat(monkeypatch, case, variant):
    """(the searches of K.CUDA_OWN_CONSTANTS read the file's own constants: there the device must
    ignore lbfgs_constants as the oracle does)"""
    r = solve(monkeypatch, case, cuda_compat=True, cuda_variant=variant)
    o = K.oracle(case, cuda=2 if variant else 1)
    check_oracle(r, o, (case, variant))


# ---- 10. emulated sharding ------------------------------------------------------------------------
def test_sharded_emulated(monkeypatch):
    """two emulated ranks, every rank owning segments: the one-rank run's bits with the same constants"""
    ks, obj, n, m, ls, iters = K.SHARDED
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    x0 = L.x0_uniform(n, K.SEED, K.LO, K.HI)
    kc = K.device_constants(L, ks)
    with L.Context(n, m) as c:
        ref = c.minimize(obj, x0, ls, iters, tolerance=K.TOL, trace=True, consts=kc)
    assert np.any(ref["tr_alpha"][~np.isnan(ref["tr_alpha"])] > K.SETS[ks]["initial_step"])
    world = 2
    grp = L.HostGroup(world)
    ctxs = [L.Context(n, m, rank=r, group=grp) for r in range(world)]
    out, err = [None] * world, [None] * world

    def run(r):
        try:
            out[r] = ctxs[r].minimize(obj, x0, ls, iters, tolerance=K.TOL, trace=True, consts=kc)
        except Exception as e:  # pragma: no cover
            err[r] = e

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not any(err), err
    x = np.zeros(n)
    for r in range(world):
        for key in ("tr_f", "tr_gnorm"):
            assert np.array_equal(bits(out[r][key]), bits(ref[key])), (r, key)
        assert same_bits(out[r]["tr_alpha"], ref["tr_alpha"]), r
        assert np.array_equal(out[r]["tr_c1"], ref["tr_c1"]) and np.array_equal(out[r]["tr_c2"], ref["tr_c2"]), r
        assert out[r]["status"] == ref["status"] and out[r]["iterations"] == ref["iterations"], r
        assert out[r]["messages"] == ref["messages"], r
        lo, nl = ctxs[r].elem_lo, ctxs[r].n_loc
        assert nl > 0
        x[lo:lo + nl] = out[r]["x"][lo:lo + nl]
    assert np.array_equal(bits(x), bits(ref["x"]))
    for c in ctxs:
        c.close()
    grp.close()
