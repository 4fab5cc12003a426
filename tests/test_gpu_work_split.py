"""Split work vector (LBFGS_WORK_SPLIT): the in-place two-loop passes update the end
windows of q / r in place and ping-pong the middle segments between the pass's buffer and the
context's alternate buffer; k_mid, k_last, the TWOLOOP commit and trials read through the same
per-workgroup select, and every other entry point has a displaced middle copied back first. The
select only chooses a pointer, so every setting gives the same bits:
  LBFGS_WORK_SPLIT=0             off (the baseline here)
  LBFGS_WORK_SPLIT=Wlo:Whi       the end windows, in segments
  LBFGS_WORK_SPLIT=...,poison    and the stale copy of the middle is filled with NaN after every
                                 split pass: a reader that was missed shows up as NaN instead of a
                                 plausible vector from two passes earlier
  LBFGS_WORK_SPLIT_NT=0/1        the middle's cache policy
Sizes: n = 70 001 is 35 segments of 2048 with a masked last segment of 369 elements (not a multiple
of 128), n = 1000 is two segments of 512 (the second masked); both with LBFGS_COOP=0, so that the
launch sequence runs. n = 2 361 601 takes the launch sequence on its own (4613 segments, both walks).
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

COOP_RANGE = 524288  # at and below: LBFGS_COOP=0, so that the launch sequence runs
N = 70_001           # 35 segments
# windows (low:high end, in segments) at N -> what they exercise
WINDOWS = {
    "17:17": "a middle of exactly one segment (17)",
    "2:0": "the masked last segment inside the middle",
    "3:2": "the masked last segment inside a window",
    "18:18": "windows covering everything: no middle, today's path",
}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def setup_env(monkeypatch, n, split, nt=0, rev=None):
    monkeypatch.setenv("LBFGS_WORK_SPLIT", split)
    monkeypatch.setenv("LBFGS_WORK_SPLIT_NT", str(nt))
    if rev is None:
        monkeypatch.delenv("LBFGS_REV", raising=False)
    else:
        monkeypatch.setenv("LBFGS_REV", str(rev))
    if n <= COOP_RANGE:
        monkeypatch.setenv("LBFGS_COOP", "0")


def solve(monkeypatch, n, m, obj, ls, iters, x0, split, nt=0, rev=None, **kw):
    """one solve; the split counters' growth rides along"""
    setup_env(monkeypatch, n, split, nt, rev)
    before = L.Context.work_split_stats()
    with np.errstate(all="ignore"), L.Context(n, m) as c:
        r = c.minimize(obj, x0, ls, iters, trace=True, **kw)
    after = L.Context.work_split_stats()
    r["ws"] = {k: after[k] - before[k] for k in after}
    return r


def same(a, b):
    for key in ("tr_f", "tr_gnorm", "tr_c1", "tr_c2", "x"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    ta, tb = a["tr_alpha"], b["tr_alpha"]
    assert np.array_equal(np.isnan(ta), np.isnan(tb)) and np.array_equal(bits(ta[~np.isnan(ta)]), bits(tb[~np.isnan(tb)]))
    assert a["messages"] == b["messages"] and a["status"] == b["status"] and a["iterations"] == b["iterations"]


def same_as_oracle(r, o):
    assert np.array_equal(bits(r["tr_f"]), bits(o["f"])) and np.array_equal(bits(r["tr_gnorm"]), bits(o["gnorm"]))
    assert np.array_equal(r["tr_c1"], o["c1"]) and np.array_equal(r["tr_c2"], o["c2"])
    assert np.array_equal(bits(r["x"]), bits(o["x"]))
    ta, tb = r["tr_alpha"], o["alpha"]
    assert np.array_equal(np.isnan(ta), np.isnan(tb)) and np.array_equal(bits(ta[~np.isnan(ta)]), bits(tb[~np.isnan(tb)]))


_oracle = {}


def oracle(obj, x0, ls, m, iters, tol=1e-5):
    key = (obj, len(x0), ls, m, iters, tol)
    if key not in _oracle:
        with np.errstate(all="ignore"):
            _oracle[key] = O.lbfgs(obj, x0, ls, m, iters, tol, mode=O.CANON)
    return _oracle[key]


# m = 1..5 from an empty history: every h from 0 up, both parities of both loops' lengths (h = 1: no
# in-place pass; h = 2: one r pass, r displaced at the commit; h = 3: one q pass, q displaced at
# k_mid; ...). Backtracking: the commit with its candidate step, trials and recommits; Wolfe: trials
# with g.d and k_last's materialised d read a split r.
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("ls,obj", [("backtracking", "rosenbrock"), ("wolfe", "quad_tridiag")])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_split_bit_identical(monkeypatch, m, ls, obj, rev):
    iters = 8
    x0 = L.x0_uniform(N, 11, -2.0, 2.0)
    off = solve(monkeypatch, N, m, obj, ls, iters, x0, "0", rev=rev)
    assert off["ws"] == dict(passes=0, copies=0, alloc_failed=0, given_up=0)
    same_as_oracle(off, oracle(obj, x0, ls, m, iters))
    for win in WINDOWS:
        # both policies under poison, and the plain knob
        for split, nt in ((win + ",poison", 0), (win + ",poison", 1), (win, 0)):
            r = solve(monkeypatch, N, m, obj, ls, iters, x0, split, nt=nt, rev=rev)
            print(m, ls, "rev", rev, split, "nt", nt, r["ws"], "iterations", r["iterations"])
            same(off, r)
            assert r["ws"]["copies"] == 0 and r["ws"]["alloc_failed"] == 0  # no consolidation in a plain solve
            if win == "18:18" or m == 1:
                assert r["ws"]["passes"] == 0  # no middle / no in-place pass
            else:
                assert r["ws"]["passes"] > 0


def test_two_segments_middle_is_the_masked_one(monkeypatch):
    """n = 1000: two segments, window 1:0 - the middle is the masked last segment alone, and the
    commit's halo at the boundary crosses from the window's buffer into the middle's."""
    n, m, iters = 1000, 5, 12
    x0 = L.x0_uniform(n, 11, -2.0, 2.0)
    off = solve(monkeypatch, n, m, "rosenbrock", "backtracking", iters, x0, "0")
    same_as_oracle(off, oracle("rosenbrock", x0, "backtracking", m, iters))
    for split, nt in (("1:0,poison", 0), ("0:1,poison", 1), ("0:0,poison", 0)):
        r = solve(monkeypatch, n, m, "rosenbrock", "backtracking", iters, x0, split, nt=nt)
        same(off, r)
        assert r["ws"]["passes"] > 0 and r["ws"]["copies"] == 0


def test_launch_sequence_size(monkeypatch):
    """The smallest kind of n that takes the launch sequence on its own: 4613 segments, a tail group
    of 7, a last segment of one element; the default walk (reversed every other pass)."""
    n, m, iters = 2_361_601, 4, 6
    x0 = L.x0_uniform(n, 11, -2.0, 2.0)
    off = solve(monkeypatch, n, m, "rosenbrock", "backtracking", iters, x0, "0")
    for split, nt in (("400:0,poison", 1), ("1000:1000,poison", 0)):
        r = solve(monkeypatch, n, m, "rosenbrock", "backtracking", iters, x0, split, nt=nt)
        same(off, r)
        assert r["ws"]["passes"] > 0 and r["ws"]["copies"] == 0


def test_not_a_descent_direction(monkeypatch):
    """At the separable quadratic's minimum every two-loop direction is 0: "Not a descent direction",
    and the NEG_G commit follows a TWOLOOP commit that read a split r (tolerance 0 lets the
    iterations run on)."""
    m, iters = 4, 8
    x0 = L.x0_uniform(N, 11, -2.0, 2.0)
    off = solve(monkeypatch, N, m, "quad_sep", "interpolation", iters, x0, "0", tolerance=0.0)
    assert "Not a descent direction" in off["messages"]
    same_as_oracle(off, oracle("quad_sep", x0, "interpolation", m, iters, 0.0))
    for split, nt in (("3:2,poison", 0), ("2:0,poison", 1)):
        r = solve(monkeypatch, N, m, "quad_sep", "interpolation", iters, x0, split, nt=nt, tolerance=0.0)
        same(off, r)
        assert r["ws"]["copies"] == 0


def run_steps(monkeypatch, split, nt, m, k):
    """two solves on one context, the second init on the live context (a reset), each with a
    download of x in the middle of the solve"""
    setup_env(monkeypatch, N, split, nt)
    xa, xb = L.x0_uniform(N, 11, -2.0, 2.0), L.x0_uniform(N, 12, -1.5, 1.5)
    before = L.Context.work_split_stats()
    got = []
    with L.Context(N, m) as c:
        for x0 in (xa, xb, xa):
            c.init("rosenbrock", x0, "backtracking", trace=True)
            c.step(k)
            xm = bits(c.get_x()).copy()  # mid-solve
            r = c.step(k)
            t = c.trace()
            got.append((r["f"], r["gnorm"], r["iterations"], xm, bits(c.get_x()).copy(), bits(t["tr_f"]).copy(),
                        t["tr_c1"].copy(), t["tr_c2"].copy()))
    after = L.Context.work_split_stats()
    return got, {key: after[key] - before[key] for key in after}


@pytest.mark.parametrize("m", [2, 3])  # r displaced at the end of an iteration / whole
def test_reset_and_download(monkeypatch, m):
    """A second init on a live context and a download of x between steps. x is never a split vector,
    so its download needs no copy; the init's upload ends the split state, copying a displaced
    middle back (h - 1 odd: r is displaced when the iteration ends) - the only consolidation copies
    of the suite's solves."""
    k = 4
    off, ws_off = run_steps(monkeypatch, "0", 0, m, k)
    assert ws_off["passes"] == 0 and ws_off["copies"] == 0
    for split, nt in (("3:2,poison", 0), ("2:0,poison", 1)):
        got, ws = run_steps(monkeypatch, split, nt, m, k)
        print(m, split, ws)
        for a, b in zip(off, got):
            assert a[:3] == b[:3]
            for u, v in zip(a[3:], b[3:]):
                assert np.array_equal(u, v)
        assert ws["passes"] > 0 and ws["alloc_failed"] == 0
        # at most one copy per init after the first (none where the iteration ends with r whole)
        assert ws["copies"] <= 2
        if m == 2:
            assert ws["copies"] == 2
    # the same start gives the same solve, whatever the context held before
    assert off[0][:3] == off[2][:3] and np.array_equal(off[0][4], off[2][4])
