"""The GPU cases of tests/test_gpu_batch_device.py, which runs this file in a process of its own
(torch is imported before the library is loaded, so that both use one HIP runtime).

The batched solver with x0, x, A and b in device memory (lbfgs_batch_minimize_device,
lbfgs_batch_set_dense_quadratics_device, Batch.minimize_device, Batch.set_dense_quadratics_device).
Every comparison is by bits (same_bits' NaN rule). The references are the canonical-order oracle,
run once per problem on the CPU, and the host forms of the same Batch object. Every case first
asserts on the CPU what it needs from the oracle. Input buffers are NaN-filled allocations with the
rows written into them, so a read outside a row poisons a result; output buffers are filled with a
finite sentinel and every element outside the rows is checked unchanged afterwards.

Shapes are the smallest at which the indexing can go wrong. Stencil: n = 5 (one segment), 513 (a
second segment of one element), 1537 (several segments). Dense: n = 3 (fewer rows than waves), 65
(one lane stride plus one element), 100 (a partial second lane stride). m = 1 and 5, B = 3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  before lbfgs_amd loads liblbfgs_hip.so: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import lbfgs_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import test_gpu_batch as S  # noqa: E402  (the stencil batch's oracle cache)
import test_gpu_batch_dense as D  # noqa: E402  (fixture_batch, spectrum_batch, oracle, check_problem, same_bits)

pytestmark = pytest.mark.gpu

BAD_ARG = -1
SENTINEL = 1234.5
DEV = "cuda:0"
same_bits = D.same_bits
RESULT_KEYS = ("f", "gnorm", "iterations", "status_code", "trials_f", "trials_fg", "commits", "h_min", "h_max", "bytes")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


# ---- buffers -------------------------------------------------------------------------------------
def rows(data, ld, offset=0, fill=float("nan"), tail=3):
    """(allocation, view): the rows of `data` (2-D) at stride ld from storage offset `offset` of an
    allocation filled with `fill`; ld = 0: one row, expanded."""
    data = np.ascontiguousarray(data, np.float64)
    B, n = data.shape
    buf = torch.full((offset + (B - 1) * ld + n + tail,), fill, dtype=torch.float64, device=DEV)
    if ld == 0:
        assert all(np.array_equal(data[0], r) for r in data)
        buf[offset:offset + n] = dev(data[0])
        return buf, buf[offset:offset + n].unsqueeze(0).expand(B, n)
    view = buf.as_strided((B, n), (ld, 1), offset)
    view.copy_(dev(data))
    return buf, view


def matrices(A, lda, astride, offset=0):
    """(allocation, view) of A (B x n x n, or n x n) at row stride lda and batch stride astride in a
    NaN-filled allocation"""
    A = np.ascontiguousarray(A, np.float64)
    n = A.shape[-1]
    nb = A.shape[0] if A.ndim == 3 else 1
    buf = torch.full((offset + (nb - 1) * astride + (n - 1) * lda + n + 3,), float("nan"), dtype=torch.float64,
                     device=DEV)
    if A.ndim == 2:
        view = buf.as_strided((n, n), (lda, 1), offset)
    else:
        view = buf.as_strided((nb, n, n), (astride, lda, 1), offset)
    view.copy_(dev(A))
    return buf, view


def outside_unchanged(buf, B, n, ld, offset, fill=SENTINEL):
    """every element of the allocation outside the rows still holds the fill"""
    h = host(buf)
    inside = np.zeros(h.shape, bool)
    for p in range(B):
        inside[offset + p * ld:offset + p * ld + n] = True
    rest = h[~inside]
    return bool(np.isnan(rest).all()) if np.isnan(fill) else bool(np.array_equal(rest, np.full(rest.shape, fill)))


def on_host(res):
    r = dict(res)
    r["x"] = host(res["x"])
    return r


def same_result(rd, rh, what):
    """a device-form result against a host-form one of the same Batch: everything but the call's seconds"""
    assert same_bits(host(rd["x"]) if hasattr(rd["x"], "cpu") else rd["x"], rh["x"]), what
    for k in RESULT_KEYS:
        assert same_bits(np.asarray(rd[k], np.float64), np.asarray(rh[k], np.float64)), (what, k, rd[k], rh[k])
    assert rd["status"] == rh["status"] and rd["launches"] == rh["launches"], what
    for p in range(len(rh["tr_f"])):
        for k in ("tr_f", "tr_gnorm", "tr_alpha"):
            assert same_bits(rd[k][p], rh[k][p]), (what, k, p)
        assert rd["events"][p] == rh["events"][p], (what, p)


# ---- 1. stencil objectives, every stride form -------------------------------------------------------
FORMS = ["contiguous", "padded_offset", "broadcast", "in_place"]
NS, MS = [5, 513, 1537], [1, 5]
STENCIL = []
for oi, obj in enumerate(S.OBJS):
    for fi, form in enumerate(FORMS):
        i = oi * len(FORMS) + fi  # every form with every objective; (n, m): all six, twice; a search
        STENCIL.append((obj, form, S.SEARCHES[(oi + fi) % 4], NS[i % 3], MS[(i // 3) % 2]))  # moves with the form
assert {s for o, f, s, n, m in STENCIL if f != "contiguous"} == set(S.SEARCHES)
assert {(n, m) for o, f, s, n, m in STENCIL} == {(n, m) for n in NS for m in MS}


def stencil_x0(n, form, B=3):
    if form == "broadcast":
        return np.stack([O.x0_uniform(n, 1, -2.0, 2.0)] * B)
    # problems that end at different times: far starts, one beside the vector of ones, that vector itself
    far = [O.x0_uniform(n, 1 + q, -2.0, 2.0) for q in range(B - 2)]
    return np.stack(far + [1.0 + O.x0_uniform(n, 4, -1e-4, 1e-4), np.ones(n)])


def x0_and_out(X0, form):
    """the input view and the output (allocation, view, ld, offset, fill) of a stride form"""
    B, n = X0.shape
    if form == "contiguous":
        xin = rows(X0, n, 0, tail=0)[1]
        assert xin.is_contiguous()
        ld, off = n, 0
    elif form == "padded_offset":
        xin = rows(X0, n + 1, 1)[1]  # rows only 8-byte aligned
        ld, off = n + 1, 1
    elif form == "broadcast":
        xin = rows(X0, 0, 1)[1]
        assert xin.stride() == (0, 1)
        ld, off = n + 1, 1
    else:  # the result over x0, in a padded allocation
        buf, xin = rows(X0, n + 3, 1)
        return xin, (buf, xin, n + 3, 1, float("nan"))
    buf, out = rows(np.full((B, n), SENTINEL), ld, off, fill=SENTINEL)
    return xin, (buf, out, ld, off, SENTINEL)


@pytest.mark.parametrize("obj,form,ls,n,m", STENCIL)
def test_stencil_rows(obj, form, ls, n, m):
    B, maxit = 3, 12
    X0 = stencil_x0(n, form)
    orc = S.oracle(obj, X0, ls, m, maxit, 1e-5, ("dev", obj, form, ls, n, m))
    iters = [o["iters"] for o in orc]  # conditions on the inputs (CPU)
    assert all(o["status"] in ("converged", "max_iter") for o in orc), [o["status"] for o in orc]
    assert form == "broadcast" or len(set(iters)) >= 2, iters
    xin, (buf, out, ld, off, fill) = x0_and_out(X0, form)
    with L.Batch(n, m, B) as bt:
        rh = bt.minimize(obj, X0, ls, max_iterations=maxit, tolerance=1e-5, trace=True)
        rd = bt.minimize_device(obj, xin, ls, max_iterations=maxit, tolerance=1e-5, trace=True, out=out)
    assert rd["x"] is out and outside_unchanged(buf, B, n, ld, off, fill), (obj, form)
    if form != "in_place":
        assert same_bits(host(xin), X0)  # x0 is only read
    same_result(rd, rh, (obj, form, ls, n, m))
    r = on_host(rd)
    for p in range(B):
        D.check_problem(r, p, orc[p], (obj, form, ls, n, m))


# ---- 2. dense quadratics by reference, every stride form ---------------------------------------------
DENSE_FORMS = ["contiguous", "padded", "shared_expand", "shared_2d_shared_b"]
DENSE = []
for ni, n in enumerate([3, 65, 100]):
    for fi, form in enumerate(DENSE_FORMS):
        DENSE.append((n, form, S.SEARCHES[(ni + fi) % 4], MS[(ni + fi) % 2]))


def dense_data(n, form, B=3):
    """A, b, X0, the iteration limit and the status the oracle is to end with"""
    if f"mat{n}" in D._data.files:
        A, b, X0 = D.fixture_batch(n, B)
        maxit, status = 1000, "converged"
    else:
        A, b, X0 = D.spectrum_batch(n, B, np.logspace(0, 3, n), 1000 + n)
        maxit, status = 14, "max_iter"
    if form.startswith("shared"):
        A = np.ascontiguousarray(A[1])
    if form.endswith("shared_b"):
        b = np.stack([b[1]] * B)
    return A, b, X0, maxit, status


def dense_tensors(A, b, form):
    n = A.shape[-1]
    if form == "contiguous":
        At, bt_ = matrices(A, n, n * n)[1], rows(b, n)[1]
    elif form == "padded":
        At, bt_ = matrices(A, n + 3, n * (n + 3) + 5, 1)[1], rows(b, n + 1, 1)[1]
    elif form == "shared_expand":
        At, bt_ = matrices(A, n + 3, 0, 1)[1].unsqueeze(0).expand(len(b), n, n), rows(b, n)[1]
        assert At.stride(0) == 0
    else:
        At, bt_ = matrices(A, n, 0)[1], rows(b, 0, 1)[1]
        assert At.dim() == 2 and bt_.stride(0) == 0
    return At, bt_


@pytest.mark.parametrize("n,form,ls,m", DENSE)
def test_dense_rows(n, form, ls, m):
    B = 3
    A, b, X0, maxit, status = dense_data(n, form)
    orc = D.oracle(("dev", n, form, ls, m), A, b, X0, ls, m, maxit, 1e-5)
    iters = [orc[p]["iters"] for p in range(B)]  # conditions on the inputs (CPU)
    assert all(orc[p]["status"] == status for p in range(B)), (n, form, [orc[p]["status"] for p in range(B)])
    assert status == "max_iter" or len(set(iters)) >= 2, iters
    At, bt_ = dense_tensors(A, b, form)
    xin = rows(X0, n + 1, 1)[1]
    buf, out = rows(np.full((B, n), SENTINEL), n + 2, 1, fill=SENTINEL)
    with L.Batch(n, m, B) as bt:
        bt.set_dense_quadratics_device(At, bt_)
        rd = bt.minimize_device("dense", xin, ls, max_iterations=maxit, tolerance=1e-5, trace=True, out=out)
        assert outside_unchanged(buf, B, n, n + 2, 1)
        x_dev = host(out)
        r_mixed = bt.minimize("dense", X0, ls, max_iterations=maxit, tolerance=1e-5, trace=True)  # host x, referenced A
        bt.set_dense_quadratics(A, b)
        rh = bt.minimize("dense", X0, ls, max_iterations=maxit, tolerance=1e-5, trace=True)
        out.fill_(SENTINEL)
        r_mixed2 = bt.minimize_device("dense", xin, ls, max_iterations=maxit, tolerance=1e-5, trace=True, out=out)
    assert same_bits(host(At), A if form != "shared_expand" else np.stack([A] * B))  # A and b are only read
    assert same_bits(host(bt_), b) and same_bits(host(xin), X0)
    rd = dict(rd, x=x_dev)
    for other, what in ((rh, "host forms"), (r_mixed, "host x, referenced A"), (on_host(r_mixed2), "device x, copied A")):
        same_result(rd, other, (n, form, ls, m, what))
    for p in range(B):
        D.check_problem(rd, p, orc[p], (n, form, ls, m))


# ---- 3. by reference ---------------------------------------------------------------------------------
def test_by_reference():
    n, m, B, ls = 10, 3, 3, "interpolation"
    A1, b1, X0 = D.fixture_batch(n, B)
    A2, b2 = A1[::-1] + 0.5 * np.eye(n), 2.0 * b1[::-1]
    sep = np.stack([O.x0_uniform(n, 7 + p, -2.0, 2.0) for p in range(B)])
    orc1 = D.oracle(("devref", 1), A1, b1, X0, ls, m, 1000, 1e-5)
    orc2 = D.oracle(("devref", 2), A2, b2, X0, ls, m, 1000, 1e-5)
    o3 = S.oracle("quad_sep", sep, "backtracking", m, 6, 1e-5, ("devref", 3))
    assert all(o[p]["status"] == "converged" for o in (orc1, orc2) for p in range(B))  # conditions on the inputs
    assert [orc1[p]["iters"] for p in range(B)] != [orc2[p]["iters"] for p in range(B)]
    At, bt_ = matrices(A1, n + 3, n * (n + 3) + 5, 1)[1], rows(b1, n + 1, 1)[1]
    xin = dev(X0)
    kw = dict(max_iterations=1000, tolerance=1e-5, trace=True)

    def check(res, orc, what):
        r = on_host(res)
        for p in range(B):
            D.check_problem(r, p, orc[p], what)

    with L.Batch(n, m, B) as bt:
        bt.set_dense_quadratics_device(At, bt_)
        assert bt._dq_refs[0] is At and bt._dq_refs[1] is bt_  # kept alive by the object
        check(bt.minimize_device("dense", xin, ls, **kw), orc1, "first data")
        At.copy_(dev(A2))  # the same memory, other data, no setter call
        bt_.copy_(dev(b2))
        check(bt.minimize_device("dense", xin, ls, **kw), orc2, "data overwritten in place")
        bt.set_dense_quadratics(A1, b1)  # the host form: the batch's own copies again
        assert bt._dq_refs is None
        At.fill_(float("nan"))  # no longer read
        check(bt.minimize_device("dense", xin, ls, **kw), orc1, "host setter after the device setter")
        At.copy_(dev(A2))
        bt.set_dense_quadratics_device(At, bt_)
        check(bt.minimize_device("dense", xin, ls, **kw), orc2, "device setter again")
        st = on_host(bt.minimize_device("quad_sep", dev(sep), "backtracking", max_iterations=6, trace=True))
        for p in range(B):
            D.check_problem(st, p, o3[p], "a stencil solve after a by-reference dense one")
        check(bt.minimize_device("dense", xin, ls, **kw), orc2, "and dense again")
    assert bt._dq_refs is None  # close() lets go of the tensors


# ---- 4. launch shapes and streams ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["stencil_in_place", "dense"])
def test_launch_shape_does_not_matter(kind):
    B, m = 7, 3
    if kind == "dense":
        n, obj, ls = 10, "dense", "wolfe"
        A, b, X0 = D.fixture_batch(n, B)
        orc = D.oracle(("devshape",), A, b, X0, ls, m, 1000, 1e-5)
        orc = [orc[p] for p in range(B)]
        At, bt_ = dense_tensors(A, b, "padded")
    else:
        n, obj, ls = 513, "quad_tridiag", "wolfe"
        X0 = np.stack([O.x0_uniform(n, 1, -2.0, 2.0), O.x0_uniform(n, 2, -1e-3, 1e-3), O.x0_uniform(n, 3, -30.0, 30.0),
                       np.ones(n), np.zeros(n), 1.0 + O.x0_uniform(n, 4, -1e-4, 1e-4), O.x0_uniform(n, 5, -2.0, 2.0)])
        orc = S.oracle(obj, X0, ls, m, 25, 1e-5, ("devshape", kind))
    maxit = 1000 if kind == "dense" else 25
    assert len(set(o["iters"] for o in orc)) >= 3, [o["iters"] for o in orc]  # a condition on the inputs (CPU)
    results = []
    for launch in [(0, 0), (2, 3)]:  # two workgroups take the seven problems in turn, three iterations a launch
        with L.Batch(n, m, B) as bt:
            bt.set_launch(*launch)
            if kind == "dense":
                bt.set_dense_quadratics_device(At, bt_)
                xin = rows(X0, n + 1, 1)[1]
                res = bt.minimize_device(obj, xin, ls, max_iterations=maxit, trace=True)
            else:  # in place: a row is written when its problem ends, while later problems' rows are yet to be read
                buf, xin = rows(X0, n + 3, 1)
                res = bt.minimize_device(obj, xin, ls, max_iterations=maxit, trace=True, out=xin)
                assert res["x"] is xin and outside_unchanged(buf, B, n, n + 3, 1, float("nan"))
        r = on_host(res)
        for p in range(B):
            D.check_problem(r, p, orc[p], (kind, launch))
        results.append(r)
    assert results[1]["launches"] > results[0]["launches"]
    for k in ("x",) + RESULT_KEYS:
        assert same_bits(np.asarray(results[0][k], np.float64), np.asarray(results[1][k], np.float64)), k


def test_tensors_from_a_side_stream():
    n, m, B, ls = 65, 5, 3, "backtracking"
    A, b, X0, maxit, status = dense_data(n, "contiguous")
    orc = D.oracle(("devstream",), A, b, X0, ls, m, maxit, 1e-5)
    assert all(orc[p]["status"] == status for p in range(B))
    Ah, bh, Xh = (torch.from_numpy(0.5 * a).pin_memory() for a in (A, b, X0))
    side = torch.cuda.Stream(device=DEV)
    with L.Batch(n, m, B) as bt, torch.cuda.stream(side):
        # produced by kernels queued on the side stream; the binding waits for the current stream
        At = Ah.to(DEV, non_blocking=True) * 2.0
        bt_ = bh.to(DEV, non_blocking=True) * 2.0
        xin = Xh.to(DEV, non_blocking=True) * 2.0
        bt.set_dense_quadratics_device(At, bt_)
        res = bt.minimize_device("dense", xin, ls, max_iterations=maxit, trace=True)
    r = on_host(res)
    for p in range(B):
        D.check_problem(r, p, orc[p], "side stream")


# ---- 5. refusals: a status or an exception, nothing launched --------------------------------------------
def test_refusals():
    n, m, B = 5, 2, 3
    A, b, X0 = D.fixture_batch(n, B)
    orc = D.oracle(("devrefuse",), A, b, X0, "backtracking", m, 1000, 1e-5)
    lib, k = L.lib(), L.constants()
    ROS, DENSE_OBJ, BT = L.OBJECTIVES["rosenbrock"], L.OBJECTIVES["dense"], L.LINE_SEARCHES["backtracking"]
    with L.Batch(n, m, B) as bt:
        xin = dev(X0)
        buf, out = rows(np.full((B, n), SENTINEL), n + 1, 1, fill=SENTINEL)
        At, bt_ = dev(A), dev(b)
        pinned = torch.full((B * n * n + 8,), 1.0, dtype=torch.float64).pin_memory()
        assert pinned.is_pinned()

        def untouched():
            return outside_unchanged(buf, 0, n, n + 1, 1) and same_bits(host(xin), X0) and same_bits(host(At), A)

        def c_minimize(x0, ldx0, x, ldx, obj=ROS):
            res = (L.Result * B)()
            rc = lib.lbfgs_batch_minimize_device(bt.h, obj, BT, C.byref(k), x0, ldx0, x, ldx, 10, 1e-5, L.FLAG_QUIET, res)
            assert rc == BAD_ARG and lib.lbfgs_batch_last_error(bt.h), (x0, ldx0, x, ldx)
            assert untouched()

        def c_setter(a, astride, lda, bb, ldb):
            rc = lib.lbfgs_batch_set_dense_quadratics_device(bt.h, a, astride, lda, bb, ldb)
            assert rc == BAD_ARG and lib.lbfgs_batch_last_error(bt.h), (a, astride, lda, bb, ldb)

        def refused(exc, fn, *a, **kw):
            with pytest.raises(exc) as e:
                fn(*a, **kw)
            if exc is L.LbfgsError:
                assert e.value.rc == BAD_ARG
            assert untouched()

        X, Y = xin.data_ptr(), out.data_ptr()
        # null pointers and strides, at the C level
        c_minimize(None, n, Y, n + 1)
        for ldx0 in (n - 1, 1, -n):
            c_minimize(X, ldx0, Y, n + 1)
        for ldx in (n - 1, 0, -n):
            c_minimize(X, n, Y, ldx)
        c_minimize(X + 4, n, Y, n + 1)  # not 8-byte aligned
        c_minimize(X, n, Y, n + 1, obj=DENSE_OBJ)  # dense before any data is set
        c_setter(None, n * n, n, bt_.data_ptr(), n)
        c_setter(At.data_ptr(), n * n, n, None, n)
        c_setter(At.data_ptr(), n * n, n - 1, bt_.data_ptr(), n)
        c_setter(At.data_ptr(), n * n - 1, n, bt_.data_ptr(), n)
        c_setter(At.data_ptr(), n * n, n, bt_.data_ptr(), n - 1)
        # pinned host memory is visible to the device: refused by its kind, not found out by a fault
        P = pinned.data_ptr()
        c_minimize(P, n, Y, n + 1)
        c_minimize(X, n, P, n)
        c_setter(P, n * n, n, bt_.data_ptr(), n)
        c_setter(At.data_ptr(), n * n, n, P, n)
        assert bool((pinned == 1.0).all())
        c_minimize(X, n, Y, n + 1, obj=DENSE_OBJ)  # a refused setter sets nothing
        # the binding
        refused(ValueError, bt.minimize_device, "rosenbrock", xin, out=buf.as_strided((B, n), (n - 1, 1), 1))
        refused(ValueError, bt.minimize_device, "rosenbrock", xin.t().contiguous().t())  # last stride not 1
        refused(ValueError, bt.minimize_device, "rosenbrock", xin[:2])
        refused(ValueError, bt.minimize_device, "rosenbrock", xin.cpu())
        refused(TypeError, bt.minimize_device, "rosenbrock", xin.float())
        refused(TypeError, bt.minimize_device, "rosenbrock", X0)
        refused(TypeError, bt.minimize_device, "rosenbrock", xin, out=out.float())
        refused(L.LbfgsError, bt.minimize_device, "dense", xin, out=out)
        refused(TypeError, bt.set_dense_quadratics_device, At.float(), bt_)
        refused(TypeError, bt.set_dense_quadratics_device, At, bt_.float())
        refused(ValueError, bt.set_dense_quadratics_device, At.transpose(1, 2), bt_)
        refused(ValueError, bt.set_dense_quadratics_device, At[:2], bt_)
        refused(ValueError, bt.set_dense_quadratics_device, At, bt_[:, :4])
        refused(ValueError, bt.set_dense_quadratics_device, At, bt_.cpu())
        refused(L.LbfgsError, bt.minimize_device, "dense", xin, out=out)
        # overlaps: x over x0 other than identically, x over the referenced A
        both = torch.full((2 * B * n,), SENTINEL, dtype=torch.float64, device=DEV)
        x0v = both.as_strided((B, n), (n, 1), 0)
        x0v.copy_(xin)
        before = host(both)
        for shifted in (both.as_strided((B, n), (n, 1), 1), both.as_strided((B, n), (n + 1, 1), 0),
                        both.as_strided((B, n), (n, 1), B * n - 1)):
            refused(L.LbfgsError, bt.minimize_device, "rosenbrock", x0v, out=shifted)
        refused(L.LbfgsError, bt.minimize_device, "rosenbrock", x0v.as_strided((1, n), (n, 1), 0).expand(B, n), out=x0v)
        assert same_bits(host(both), before)
        bt.set_dense_quadratics_device(At, bt_)
        refused(L.LbfgsError, bt.minimize_device, "dense", xin, out=At.view(-1)[:B * n].view(B, n))
        refused(L.LbfgsError, bt.minimize_device, "dense", xin, out=bt_)
        # and the batch still works
        res = on_host(bt.minimize_device("dense", xin, "backtracking", trace=True, out=out))
        assert outside_unchanged(buf, B, n, n + 1, 1)
        for p in range(B):
            D.check_problem(res, p, orc[p], "after refusals")
    big = L.DENSE_BATCH_NMAX + 1
    with L.Batch(big, 1, 1) as bt:  # over the dense limit, as the host form
        with pytest.raises(L.LbfgsError) as e:
            bt.set_dense_quadratics_device(torch.zeros((big, big), dtype=torch.float64, device=DEV),
                                           torch.zeros((1, big), dtype=torch.float64, device=DEV))
        assert e.value.rc == BAD_ARG
