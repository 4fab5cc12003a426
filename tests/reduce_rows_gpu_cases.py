"""The GPU cases of tests/test_gpu_reduce_rows.py, which runs this file in a process of its own (torch
is imported before the library is loaded, so that both use one HIP runtime).

lbfgs_reduce_rows / lbfgs_amd.reduce_rows: the canonical fixed-order sum of every row of a table in
one launch. Everything compares bits. The references are the oracle's canonical dot (O.dot, O.CANON),
computed once per size and shared, and the single-vector reducer (Reducer.dot / .sum) on the same row.

1. against the oracle and the single reducer: n = 1, 2 (a lane pair, whole and half), 63, 64, 65 (a
   pair that straddles n), 127, 128, 129 (around a wave's 128-element row), 511, 512, 513 (around one
   segment), 1025, 1537 (two and three full segments, loaded one at a time, and one element) and the
   limit, 32767 and 32768 (64 segments, four in flight, every lane of the stage-2 wave live). B = 3, different data per row, uniform(-2, 2), in NaN-filled allocations laid out so that
   every row is 16-byte aligned, none is, or rows alternate; b per row with its own stride, and b
   shared. out sits in a sentinel-filled allocation;
2. the inputs can tell orders apart (no GPU): for n >= 513 the canonical value of every row differs
   from the plain left-to-right one, for the sum and for the dot;
3. a mask: inactive rows are all NaN and are not read, their out is not written;
4. signed zeros;
5. stream order, on a side stream and on the null stream, with no synchronisation in between;
6. 5000 rows;
7. end to end: a batch callback with f from one reduce_rows per round against the single path with
   Reducer.sum;
8. refusals through Python: ValueError, nothing launched.
"""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  before lbfgs_amd loads liblbfgs_hip.so: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import lbfgs_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import test_gpu_batch as S  # noqa: E402  (same_bits, seeds_x0)
import devobj_gpu_cases as DV  # noqa: E402  (torch_rosenbrock, torch_separable, SENTINEL)
import batchcb_gpu_cases as BC  # noqa: E402  (check_single)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = DV.SENTINEL
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025, 1537, 32767, 32768]
B1 = 3
# seed of the rows of size n: for n >= 513 chosen (the smallest k >= 0 of 5000 + 7 n + k) so that the
# canonical sum and dot of every row differ from the left-to-right ones; test_orders_differ asserts it
SEED_SHIFT = {513: 0, 1025: 2, 1537: 0, 32767: 0, 32768: 0}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def same(got, want):
    """bit for bit, no NaN expected on either side"""
    return np.array_equal(bits(got), bits(want))


_data = {}


def data(n, B=B1):
    """(a, b, canonical dot per row, canonical sum per row, canonical dot with b's row 0): computed once
    per (n, B), shared and left unchanged"""
    if (n, B) not in _data:
        rng = np.random.default_rng(5000 + 7 * n + SEED_SHIFT.get(n, 0) + 100003 * (B != B1))
        a, b = rng.uniform(-2.0, 2.0, (B, n)), rng.uniform(-2.0, 2.0, (B, n))
        one = np.ones(n)
        _data[(n, B)] = (a, b, np.array([O.dot(a[p], b[p], O.CANON) for p in range(B)]),
                         np.array([O.dot(a[p], one, O.CANON) for p in range(B)]),
                         np.array([O.dot(a[p], b[0], O.CANON) for p in range(B)]))
    return _data[(n, B)]


def table(values, ld, offset, fill=NAN):
    """values (B, n) as rows of stride ld at storage offset `offset` of a `fill`-filled allocation (the
    base of an allocation is 16-byte aligned: offset 2 is, offset 1 is not)"""
    B, n = values.shape
    big = torch.full((offset + (B - 1) * ld + n + 3,), fill, dtype=torch.float64, device=DEV)
    assert big.data_ptr() % 16 == 0
    t = big.as_strided((B, n), (ld, 1), offset)
    t.copy_(dev(values))
    return t


def shared(values, offset):
    n = len(values)
    big = torch.full((n + 4,), NAN, dtype=torch.float64, device=DEV)
    t = big[offset:offset + n]
    t.copy_(dev(values))
    return t


def aligned16(t):
    return [(t[p].data_ptr() % 16 == 0) for p in range(t.shape[0])]


def out_between(B, offset=1):
    """out at element `offset` of a sentinel-filled allocation, and the allocation"""
    big = torch.full((B + 4,), SENTINEL, dtype=torch.float64, device=DEV)
    return big[offset:offset + B], big


def outside_untouched(big, B, offset=1):
    h = host(big)
    return np.all(h[:offset] == SENTINEL) and np.all(h[offset + B:] == SENTINEL)


def layouts(n):
    """name -> ((offset, ld) of a, (offset, ld) of b or the offset of a shared b, the rows' alignment)"""
    even = n + (n & 1)
    return {
        "every row 16-byte aligned": ((2, even), (2, even), [True] * B1),
        "storage offset 1": ((1, even), (1, even), [False] * B1),
        "lda = n + 1": ((2, n + 1), (2, n + 1), None),
        "lda = n + 3": ((2, n + 3), (2, n + 3), None),
        "ldb differs": ((2, n + 1), (1, n + 2), None),
        "b shared": ((2, n + 3), 2, None),
        "b shared, 8-byte aligned": ((2, even), 1, None),
    }


# ---- 1. against the oracle and the single reducer ---------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_reduce_rows_vs_oracle_and_reducer(n):
    a, b, want_dot, want_sum, want_shared = data(n)
    seen = set()
    with L.Reducer(n) as red:
        for name, ((oa, lda), lb, align) in layouts(n).items():
            ta = table(a, lda, oa)
            assert ta.stride(0) == lda and ta.storage_offset() == oa
            if align is not None:
                assert aligned16(ta) == align, name
            seen.update(aligned16(ta))
            if isinstance(lb, tuple):
                tb, want = table(b, lb[1], lb[0]), want_dot
                assert tb.stride(0) == lb[1]
                single = [red.dot(ta[p], tb[p]) for p in range(B1)]
            else:
                tb, want = shared(b[0], lb), want_shared
                assert tb.dim() == 1 and (tb.data_ptr() % 16 == 0) == (lb == 2)
                single = [red.dot(ta[p], tb) for p in range(B1)]
            for off in (1, 2):
                out, big = out_between(B1, off)
                assert L.reduce_rows(ta, tb, out=out) is out
                got = host(out)
                assert same(got, want), (n, name, "dot", got, want)
                assert same(got, single), (n, name, "dot vs Reducer", got, single)
                assert outside_untouched(big, B1, off), (n, name)
            out, big = out_between(B1)
            L.reduce_rows(ta, out=out)
            got = host(out)
            assert same(got, want_sum), (n, name, "sum", got, want_sum)
            assert same(got, [red.sum(ta[p]) for p in range(B1)]), (n, name, "sum vs Reducer")
            assert outside_untouched(big, B1), (n, name)
            fresh = L.reduce_rows(ta, tb)  # out = None: a new tensor
            assert fresh.shape == (B1,) and fresh.dtype == torch.float64 and same(host(fresh), want)
    assert seen == {True, False}  # both load widths ran


# ---- 2. the inputs can tell orders apart ------------------------------------------------------------
def left_to_right(a, b=None):
    s = 0.0
    if b is None:
        for x in a.tolist():
            s = s + x
    else:
        for x, y in zip(a.tolist(), b.tolist()):
            s = s + x * y
    return s


def test_orders_differ():
    """On the CPU: from two segments on, the canonical order's value differs from the plain
    left-to-right one in at least one bit, in every row, for the sum and for the dot (below that they
    may agree: a few terms leave few ways to round)."""
    for n in SIZES:
        if n < 513:
            continue
        a, b, want_dot, want_sum, want_shared = data(n)
        for p in range(B1):
            assert bits([want_sum[p]])[0] != bits([left_to_right(a[p])])[0], (n, p, "sum")
            assert bits([want_dot[p]])[0] != bits([left_to_right(a[p], b[p])])[0], (n, p, "dot")
            assert bits([want_shared[p]])[0] != bits([left_to_right(a[p], b[0])])[0], (n, p, "shared b")


# ---- 3. a mask ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 513, 1537])
def test_mask(n):
    B, mask = 5, [1, 0, 1, 0, 0]
    a3, b3, want_dot, want_sum, _ = data(n)
    rows = {0: 0, 2: 1}  # active row of the table -> row of the shared data
    a, b = np.full((B, n), NAN), np.full((B, n), NAN)
    for p, q in rows.items():
        a[p], b[p] = a3[q], b3[q]
    ta, tb = table(a, n + 1, 2), table(b, n + 3, 1)
    active = torch.tensor(mask, dtype=torch.int32, device=DEV)
    for tbb, want in ((tb, want_dot), (None, want_sum)):
        out, big = out_between(B)
        L.reduce_rows(ta, tbb, active=active, out=out)
        got = host(out)
        for p in range(B):
            if p in rows:
                assert same(got[p], want[rows[p]]), (n, p, got[p], want[rows[p]])
            else:
                assert got[p] == SENTINEL, (n, p, got[p])
        assert outside_untouched(big, B)
        fresh = host(L.reduce_rows(ta, tbb, active=active))
        assert [bool(np.isnan(v)) for v in fresh] == [not m for m in mask], fresh
        assert same(fresh[[0, 2]], want[:2])
        # nothing active: nothing written
        out, big = out_between(B)
        L.reduce_rows(ta, tbb, active=torch.zeros(B, dtype=torch.int32, device=DEV), out=out)
        assert np.all(host(big) == SENTINEL)
    # any nonzero is active
    out, big = out_between(B)
    L.reduce_rows(ta, active=torch.tensor([-1, 0, 7, 0, 0], dtype=torch.int32, device=DEV), out=out)
    assert same(host(out)[[0, 2]], want_sum[:2]) and np.all(host(out)[[1, 3, 4]] == SENTINEL)


# ---- 4. signed zeros ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 513, 1537])
def test_signed_zeros(n):
    """A row of -0.0, and rows whose products are all -0.0: what the order's + 0.0 make of them is the
    single reducer's (and the oracle's) bits, whatever the sign turns out to be."""
    rng = np.random.default_rng(n)
    pos = rng.uniform(0.5, 2.0, n)
    a = np.stack([np.full(n, -0.0), np.full(n, -0.0), pos, np.zeros(n)])
    b = np.stack([np.full(n, -0.0), pos, np.full(n, -0.0), np.full(n, -0.0)])  # products: +0, -0, -0, -0
    B = len(a)
    assert np.all(np.signbit(a[1] * b[1])) and np.all(np.signbit(a[3] * b[3])) and not np.any(np.signbit(a[0] * b[0]))
    ta, tb = table(a, n + 1, 2), table(b, n + 1, 2)
    with L.Reducer(n) as red:
        want_dot = [red.dot(ta[p], tb[p]) for p in range(B)]
        want_sum = [red.sum(ta[p]) for p in range(B)]
    assert same(want_dot, [O.dot(a[p], b[p], O.CANON) for p in range(B)])
    assert same(want_sum, [O.dot(a[p], np.ones(n), O.CANON) for p in range(B)])
    got_dot, got_sum = host(L.reduce_rows(ta, tb)), host(L.reduce_rows(ta))
    assert same(got_dot, want_dot), (n, got_dot, want_dot, np.signbit(got_dot), np.signbit(want_dot))
    assert same(got_sum, want_sum), (n, got_sum, want_sum, np.signbit(got_sum), np.signbit(want_sum))
    assert np.all(got_dot == 0.0) and np.all(got_sum[[0, 1, 3]] == 0.0)


# ---- 5. streams --------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [True, False], ids=["side stream", "null stream"])
def test_stream_order(side):
    """A torch kernel fills the rows, reduce_rows follows with no synchronisation, a torch op consumes
    out: all on one stream, which alone orders them."""
    n = 1537
    a, b, want_dot, want_sum, _ = data(n)
    ha, hb = dev(a), dev(b)
    ta, tb = table(np.zeros((B1, n)), n + 1, 2), table(np.zeros((B1, n)), n + 3, 1)
    out, big = out_between(B1)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=DEV) if side else torch.cuda.default_stream(DEV)
    with torch.cuda.stream(st):
        assert (torch.cuda.current_stream().cuda_stream != 0) == side
        ta.copy_(ha * 2.0)  # kernels of this stream write the rows (an exact scaling: 2 x the sums)
        tb.copy_(hb)
        L.reduce_rows(ta, tb, out=out)
        twice = out * 0.5  # and a kernel of this stream reads the result
        sums = L.reduce_rows(ta) * 0.5
    st.synchronize()
    assert same(host(twice), want_dot), (host(twice), want_dot)
    assert same(host(sums), want_sum)
    assert outside_untouched(big, B1)


# ---- 6. many rows ------------------------------------------------------------------------------------
def test_many_rows():
    B, n = 5000, 65
    a, b, want_dot, want_sum, _ = data(n, B)
    ta, tb = table(a, n + 2, 1), table(b, n + 1, 2)
    out, big = out_between(B)
    L.reduce_rows(ta, tb, out=out)
    got = host(out)
    bad = np.flatnonzero(bits(got) != bits(want_dot))
    assert bad.size == 0, (bad[:10], got[bad[:10]], want_dot[bad[:10]])
    assert outside_untouched(big, B)
    assert same(host(L.reduce_rows(ta)), want_sum)


# ---- 7. end to end -----------------------------------------------------------------------------------
def rows_rosenbrock(calls):
    """DV.torch_rosenbrock over all rows at once, f from one reduce_rows"""
    def fn(Z, active):
        T, G = torch.zeros_like(Z), torch.zeros_like(Z)
        a, b = Z[:, :-1], Z[:, 1:]
        u = b - a * a
        T[:, :-1] = 100.0 * u * u + (1.0 - a) * (1.0 - a)
        G[:, :-1] = -400.0 * a * u - 2.0 * (1.0 - a)
        G[:, 1:] += 200.0 * u
        calls.append(1)
        return L.reduce_rows(T, active=active), G

    return fn


def rows_separable(calls):
    def fn(Z, active):
        e = Z - 1.0
        calls.append(1)
        return L.reduce_rows(e * e, active=active), 2.0 * e

    return fn


@pytest.mark.parametrize("make,rows", [(DV.torch_rosenbrock, rows_rosenbrock), (DV.torch_separable, rows_separable)],
                         ids=["rosenbrock", "separable"])
@pytest.mark.parametrize("ls", ["wolfe", "backtracking"])
def test_batch_callback_with_reduce_rows_vs_single(make, rows, ls):
    """The comparison of batchcb_gpu_cases.test_torch_objective_batch_vs_single, with the per-row loop of
    Reducer.sum replaced by one reduce_rows per round: every problem's x, f, |g|, counters and trace are
    the single path's bits."""
    n, m, B, iters = 2000, 5, 3, 30
    X0 = S.seeds_x0(n, [1, 2, 3], -2.0, 2.0)
    X0[1] *= 1e-3
    with L.Reducer(n) as red, L.Context(n, m) as c, L.Batch(n, m, B) as b:
        c.set_device_objective(make(red), eager_grad=True)
        one = []
        for x0 in X0:
            r = c.minimize_device("device", dev(x0), ls, iters, trace=True)
            r["x"] = host(r["x"])
            one.append(r)
        assert max(r["iterations"] for r in one) >= 2
        calls = []
        b.set_device_objective(rows(calls))
        ld = n + 3
        buf0 = torch.full((1 + B * ld,), NAN, dtype=torch.float64, device=DEV)
        bufx = torch.full((1 + B * ld,), SENTINEL, dtype=torch.float64, device=DEV)
        T0, TX = buf0.as_strided((B, n), (ld, 1), 1), bufx.as_strided((B, n), (ld, 1), 1)
        T0.copy_(dev(X0))
        for form in ("host", "device"):
            del calls[:]
            if form == "host":
                res = b.minimize("device", X0, ls, max_iterations=iters, trace=True)
            else:
                res = b.minimize_device("device", T0, ls, max_iterations=iters, trace=True, out=TX)
                assert res["x"] is TX
            assert len(calls) == max(res["f_calls"]) == res["launches"] - 1  # one reduce_rows per round
            for p in range(B):
                BC.check_single(res, p, one[p], (make.__name__, ls, form))
                if not np.all(np.isfinite(one[p]["tr_alpha"][:-1])):
                    assert 0 < res["f_calls"][p] <= one[p]["grad_calls"], (p, res["f_calls"][p], one[p]["grad_calls"])


# ---- 8. refusals through Python ----------------------------------------------------------------------
def test_refusals():
    B, n = 3, 100
    f64 = dict(dtype=torch.float64, device=DEV)
    ok = torch.zeros((B, n), **f64)
    launched = []
    real = L.lib().lbfgs_reduce_rows
    try:
        L.lib().lbfgs_reduce_rows = lambda *a: launched.append(a) or 0
        bad_a = {
            "float32": torch.zeros((B, n), dtype=torch.float32, device=DEV),
            "a CPU tensor": torch.zeros((B, n), dtype=torch.float64),
            "stride(1) != 1": torch.zeros((B, 2 * n), **f64)[:, ::2],
            "stride(0) < n": torch.zeros(n + B, **f64).as_strided((B, n), (1, 1)),
            "stride(0) = 0": torch.zeros(n, **f64).expand(B, n),
            "n = 32769": torch.zeros((2, 32769), **f64),
            "1-D": torch.zeros(n, **f64),
            "3-D": torch.zeros((B, n, 1), **f64),
            "no rows": torch.zeros((0, n), **f64),
            "not a tensor": np.zeros((B, n)),
        }
        for what, t in bad_a.items():
            with pytest.raises(ValueError):
                L.reduce_rows(t)
        bad_b = {
            "float32": torch.zeros((B, n), dtype=torch.float32, device=DEV),
            "a CPU tensor": torch.zeros((B, n), dtype=torch.float64),
            "another n": torch.zeros((B, n + 1), **f64),
            "another B": torch.zeros((B + 1, n), **f64),
            "shared, another n": torch.zeros(n - 1, **f64),
            "shared, strided": torch.zeros(2 * n, **f64)[::2],
            "stride(1) != 1": torch.zeros((B, 2 * n), **f64)[:, ::2],
            "stride(0) < n": torch.zeros(n + B, **f64).as_strided((B, n), (1, 1)),
            "3-D": torch.zeros((B, n, 1), **f64),
        }
        for what, t in bad_b.items():
            with pytest.raises(ValueError):
                L.reduce_rows(ok, t)
        bad_active = {
            "int64": torch.ones(B, dtype=torch.int64, device=DEV),
            "another B": torch.ones(B + 1, dtype=torch.int32, device=DEV),
            "a CPU tensor": torch.ones(B, dtype=torch.int32),
            "strided": torch.ones(2 * B, dtype=torch.int32, device=DEV)[::2],
            "2-D": torch.ones((B, 1), dtype=torch.int32, device=DEV),
        }
        for what, t in bad_active.items():
            with pytest.raises(ValueError):
                L.reduce_rows(ok, active=t)
        bad_out = {
            "float32": torch.zeros(B, dtype=torch.float32, device=DEV),
            "another B": torch.zeros(B - 1, **f64),
            "a CPU tensor": torch.zeros(B, dtype=torch.float64),
            "strided": torch.zeros(2 * B, **f64)[::2],
            "2-D": torch.zeros((B, 1), **f64),
        }
        for what, t in bad_out.items():
            with pytest.raises(ValueError):
                L.reduce_rows(ok, out=t)
        assert not launched  # nothing reached the library
        L.reduce_rows(ok, ok[0].clone(), active=torch.ones(B, dtype=torch.int32, device=DEV), out=torch.zeros(B, **f64))
        assert len(launched) == 1  # (the stand-in sees what is not refused)
    finally:
        L.lib().lbfgs_reduce_rows = real
    # the library's own refusal surfaces as LbfgsError with .rc
    with pytest.raises(L.LbfgsError) as e:
        L.lib().lbfgs_reduce_rows = lambda *a: -1
        try:
            L.reduce_rows(ok)
        finally:
            L.lib().lbfgs_reduce_rows = real
    assert e.value.rc == -1
    assert same(host(L.reduce_rows(ok)), np.zeros(B))
