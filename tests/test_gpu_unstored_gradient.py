"""Unstored gradients (LBFGS_STORE_G): on one rank's launch sequence the TWOLOOP commit
of a built-in objective forms g = grad f(x) from the x it already holds and does not store g_new
(3 R + 3 W instead of 4 R + 4 W), and the first first-loop pass forms it from x as well
(k_axpy_dot_x). Every other reader has the buffer filled first. The gradient is recomputed with the
operands and operations of the pass that would have stored it, so every setting gives the same bits:
  LBFGS_STORE_G=1       always store (the previous path, the baseline here)
  unset                 the default
  LBFGS_STORE_G=poison  the default, and an unstored gradient's buffer is filled with NaN: a reader
                        that was missed shows up as NaN instead of a plausible two-iterations-old g
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import lbfgs_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = ("1", None, "poison")
COOP_RANGE = 524288  # at and below: LBFGS_COOP=0, so that the launch sequence runs


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def setup_env(monkeypatch, store, n):
    if store is None:
        monkeypatch.delenv("LBFGS_STORE_G", raising=False)
    else:
        monkeypatch.setenv("LBFGS_STORE_G", store)
    if n <= COOP_RANGE:
        monkeypatch.setenv("LBFGS_COOP", "0")


def solve(monkeypatch, store, n, m, obj, ls, iters, x0, **kw):
    setup_env(monkeypatch, store, n)
    with np.errstate(all="ignore"), L.Context(n, m) as c:
        c.prof_reset()
        c.prof_enable(True)
        r = c.minimize(obj, x0, ls, iters, trace=True, **kw)
        c.prof_enable(False)
        r["commit_launches"] = c.prof_get("commit")["launches"]
    return r


def same(a, b):
    for key in ("tr_f", "tr_gnorm", "x"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    ta, tb = a["tr_alpha"], b["tr_alpha"]
    assert np.array_equal(np.isnan(ta), np.isnan(tb)) and np.array_equal(bits(ta[~np.isnan(ta)]), bits(tb[~np.isnan(tb)]))
    assert a["messages"] == b["messages"] and a["status"] == b["status"] and a["iterations"] == b["iterations"]


# tol: the separable quadratic is at its minimum after the first iteration's line search, so the
# default tolerance ends the solve before any TWOLOOP commit; tolerance 0 lets the iterations run on
# (at the minimum every two-loop direction is 0: "Not a descent direction", and the NEG_G commit
# follows a commit that left its gradient unstored - with a built-in objective)
@pytest.mark.parametrize("n,m,obj,ls,iters,tol", [
    (1000, 5, "rosenbrock", "backtracking", 12, 1e-5),        # L = 512: two segments, the second masked (488): memory halos
    (4099, 1, "rosenbrock", "backtracking", 12, 1e-5),        # h = 1: lbk_mid reads g, stored on touch every iteration
    (70_001, 5, "quad_tridiag", "wolfe", 10, 1e-5),           # L = 2048: one 16-row stencil step; trials with g.d; recommit
    (70_001, 7, "quad_sep", "interpolation", 8, 0.0),         # no stencil: recomputed without a halo
    (2_361_601, 5, "rosenbrock", "backtracking", 10, 1e-5),   # 4613 segments, tail group of 7, last of 1 element, both walks
    (25_000_003, 10, "rosenbrock", "backtracking", 14, 1e-5),  # L > 2048: the LDS carry; NT; collect stage 2; candidate step
])
def test_unstored_gradient_bit_identical(monkeypatch, n, m, obj, ls, iters, tol):
    x0 = L.x0_uniform(n, 11, -2.0, 2.0)
    stored, default, poison = (solve(monkeypatch, s, n, m, obj, ls, iters, x0, tolerance=tol) for s in SETTINGS)
    for r in (default, poison):
        print(n, obj, ls, "iterations", r["iterations"], "commits", r["commits"], "bytes", r["bytes"], "stored",
              stored["bytes"])
        same(stored, r)
        # the new path ran: as many commits, launched as often, over fewer bytes
        assert r["commits"] == stored["commits"] and r["commit_launches"] == stored["commit_launches"]
        assert r["bytes"] < stored["bytes"]
    if obj == "quad_sep":
        assert "Not a descent direction" in default["messages"]
    if n <= 70_001:  # and the canonical oracle, as the rest of the suite
        with np.errstate(all="ignore"):
            o = O.lbfgs(obj, x0, ls, m, iters, tol, mode=O.CANON)
        assert np.array_equal(bits(default["tr_f"]), bits(o["f"])) and np.array_equal(bits(default["x"]), bits(o["x"]))


def test_not_a_descent_direction_golden(monkeypatch):
    """A stress golden that prints "Not a descent direction", on the launch-sequence path: the
    reference's stdout in every setting. The goldens with that message are host-callback objectives,
    whose commits take their gradient from a buffer: no gradient is left unstored there, so this case
    checks that the knob leaves that path alone; the separable-quadratic case above reaches the
    message with a built-in objective."""
    name = "stress_tiny_sq_btw"
    meta, _ = O.load_golden(name)
    assert "Not a descent direction" in meta["stdout"]
    n = meta["n"]
    x0 = O.x0_uniform(n, meta["seed"], meta["lo"], meta["hi"])
    f, grad = O.stress_objective(meta["objective"])
    out = [solve(monkeypatch, s, n, meta["m"], "host", meta["method"], meta["maxit"], x0, tolerance=meta["tol"], f=f,
                 grad=grad) for s in SETTINGS]
    for r in out:
        assert r["messages"] == meta["stdout"]
        same(out[0], r)


def test_second_init_on_a_live_context(monkeypatch):
    """A second init with a new x0 between two solves on one context: the upload overwrites the x of
    a live unstored gradient."""
    n, m, k = 70_001, 5, 7
    xa, xb = L.x0_uniform(n, 11, -2.0, 2.0), L.x0_uniform(n, 12, -1.5, 1.5)
    out = []
    for s in SETTINGS:
        setup_env(monkeypatch, s, n)
        with L.Context(n, m) as c:
            got = []
            for x0 in (xa, xb, xa):
                c.init("rosenbrock", x0, "backtracking", trace=True)
                r = c.step(k)
                got.append((r["f"], r["gnorm"], r["iterations"], bits(c.get_x()).copy(), bits(c.trace()["tr_f"]).copy()))
        out.append(got)
    for got in out[1:]:
        for a, b in zip(out[0], got):
            assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    # the same start gives the same solve, whatever the context held before
    assert out[1][0][:3] == out[1][2][:3] and np.array_equal(out[1][0][3], out[1][2][3])


def test_other_objective_on_a_live_context(monkeypatch):
    """A host-callback solve after a built-in one on the same context: its x0 upload ends every
    entry the first solve left, so nothing of the first objective is stored into its vectors."""
    n, m = 1000, 3
    xa = L.x0_uniform(n, 11, -2.0, 2.0)
    f, grad = O.stress_objective("stress_scaled_sq")
    out = []
    for s in SETTINGS:
        setup_env(monkeypatch, s, n)
        with np.errstate(all="ignore"), L.Context(n, m) as c:
            a = c.minimize("rosenbrock", xa, "backtracking", 9, trace=True)
            b = c.minimize("host", xa, "backtracking", 6, tolerance=0.0, f=f, grad=grad, trace=True)
            a2 = c.minimize("rosenbrock", xa, "backtracking", 9, trace=True)
        out.append((a, b, a2))
    for got in out[1:]:
        for r0, r in zip(out[0], got):
            same(r0, r)
    same(out[1][0], out[1][2])
