"""The GPU cases of tests/test_gpu_batch_ragged_device.py, which runs this file in a process of its own
(torch is imported before the library is loaded, so that both use one HIP runtime).

Ragged batches with x0, x, A and b in device memory: padded rows, (B, W) with W >= the largest n_p
of which only [0, n_p) of row p is read or written, or one packed tensor (LBFGS_BATCH_PACKED). Every
comparison is by bits. The references are the canonical-order oracle, run once per problem on the
CPU at its own n_p, and the host forms of the same Batch object. Input buffers are NaN-filled
allocations with the data written into them, so a read past n_p poisons a result; output buffers are
filled with a finite sentinel and every element outside [0, n_p) of every row, and around the packed
range, is checked unchanged afterwards.

Sizes, stencil: 513 (a second segment of one element), 5, 1537, 512, 129, 1024. Dense: 3 (fewer rows
than waves), 65 (one lane stride plus one element), 100, 2."""
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

pytestmark = pytest.mark.gpu

BAD_ARG = -1
SENTINEL = 1234.5
NAN = float("nan")
DEV = "cuda:0"
OBJS = ["rosenbrock", "quad_tridiag", "quad_sep"]
SEARCHES = ["backtracking", "interpolation", "wolfe", "backtracking_wolfe"]
MESSAGES = ["Not a descent direction", "Skipping update", "Invalid rho", "Invalid gamma", "Line search failed"]
EVENT_KEYS = ["not_descent", "skipped_updates", "invalid_rho", "invalid_gamma"]
RESULT_KEYS = ("f", "gnorm", "iterations", "status_code", "trials_f", "trials_fg", "commits", "h_min", "h_max", "bytes")
SIZES = [513, 5, 1537, 512, 129, 1024]
DSIZES = [3, 65, 100, 2]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    """Equal bit for bit; a NaN equals a NaN in the same place."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def message_counts(o):
    return [sum(1 for line in o["messages"].splitlines() if m in line) for m in MESSAGES]


def check_problem(res, p, o, what=""):
    assert res["status"][p] == o["status"], (what, p, res["status"][p], o["status"])
    assert res["iterations"][p] == o["iters"], (what, p, res["iterations"][p], o["iters"])
    assert same_bits(res["x"][p], o["x"]), (what, p)
    assert same_bits([res["gnorm"][p]], [o["gnorm"][-1]]), (what, p)
    if o["status"] != "ls_failed":
        assert same_bits([res["f"][p]], [o["f"][-1]]), (what, p)
    assert same_bits(res["tr_f"][p], o["f"]) and same_bits(res["tr_gnorm"][p], o["gnorm"]), (what, p)
    a1, a2 = res["tr_alpha"][p], o["alpha"]
    assert np.array_equal(np.isnan(a1), np.isnan(a2)), (what, p)
    assert same_bits(a1[~np.isnan(a1)], a2[~np.isnan(a2)]), (what, p)
    want = message_counts(o)
    assert [res["events"][p][k] for k in EVENT_KEYS] == want[:4], (what, p, res["events"][p], want)
    assert (res["status"][p] == "ls_failed") == (want[4] > 0), (what, p)


def same_result(rd, rh, what):
    """a device-form result (x already a list of host arrays) against a host-form one of the same Batch"""
    for p in range(len(rh["x"])):
        assert same_bits(rd["x"][p], rh["x"][p]), (what, p)
        for k in ("tr_f", "tr_gnorm", "tr_alpha"):
            assert same_bits(rd[k][p], rh[k][p]), (what, k, p)
        assert rd["events"][p] == rh["events"][p], (what, p)
    for k in RESULT_KEYS:
        assert same_bits(np.asarray(rd[k], np.float64), np.asarray(rh[k], np.float64)), (what, k, rd[k], rh[k])
    assert rd["status"] == rh["status"] and rd["launches"] == rh["launches"], what


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


# ---- buffers -------------------------------------------------------------------------------------
class Buf:
    """An allocation filled with `fill` holding per-problem data: padded rows (row p's first n_p elements
    at offset + p * ld, or for matrices n_p rows lda apart from offset + p * astride) or packed."""

    def __init__(self, parts, form, fill, offset=1, pad=3, tail=3):
        parts = [np.ascontiguousarray(q, np.float64) for q in parts]
        self.sizes = [q.shape[0] for q in parts]
        self.square = parts[0].ndim == 2
        B, W = len(parts), max(self.sizes) + pad
        self.fill, self.offset, self.form = fill, offset, form
        self.inside = []
        if form == "packed":
            total = sum(q.size for q in parts)
            self.buf = torch.full((offset + total + tail,), fill, dtype=torch.float64, device=DEV)
            self.view = self.buf[offset:offset + total]
            self.view.copy_(dev(np.concatenate([q.ravel() for q in parts])))
            self.inside.append((offset, offset + total))
        elif self.square:
            self.lda, self.astride = W, W * W + 5
            self.buf = torch.full((offset + B * self.astride + tail,), fill, dtype=torch.float64, device=DEV)
            self.view = self.buf.as_strided((B, W, W), (self.astride, W, 1), offset)
            for p, q in enumerate(parts):
                self.view[p, :q.shape[0], :q.shape[0]] = dev(q)
        else:
            self.ld = W
            self.buf = torch.full((offset + B * W + tail,), fill, dtype=torch.float64, device=DEV)
            self.view = self.buf.as_strided((B, W), (W, 1), offset)
            for p, q in enumerate(parts):
                self.view[p, :q.shape[0]] = dev(q)
                self.inside.append((offset + p * W, offset + p * W + q.shape[0]))

    def parts(self):
        """the per-problem data now in the allocation (host arrays)"""
        h = host(self.buf)
        if self.form == "packed":
            cuts = np.cumsum([0] + [n * n if self.square else n for n in self.sizes]) + self.offset
            return [h[cuts[p]:cuts[p + 1]].reshape((n, n) if self.square else (n,)) for p, n in enumerate(self.sizes)]
        v = host(self.view)
        return [v[p, :n, :n] if self.square else v[p, :n] for p, n in enumerate(self.sizes)]

    def outside_unchanged(self):
        """every element of the allocation outside the problems' data still holds the fill (rows and packed)"""
        h = host(self.buf)
        mask = np.ones(h.shape, bool)
        for lo, hi in self.inside:
            mask[lo:hi] = False
        rest = h[mask]
        return bool(np.isnan(rest).all()) if np.isnan(self.fill) else bool(np.array_equal(rest, np.full(rest.shape, self.fill)))


def x0s(sizes, seed0=1):
    # problems that end at different times: far starts, one beside the vector of ones, that vector itself
    X = [O.x0_uniform(n, seed0 + p, -2.0, 2.0) for p, n in enumerate(sizes)]
    X[-2] = 1.0 + O.x0_uniform(sizes[-2], 4, -1e-4, 1e-4)
    X[-1] = np.ones(sizes[-1])
    return X


def with_host_x(res, out):
    r = dict(res)
    r["x"] = out.parts()
    return r


_oracle = {}


def oracle(key, obj, X0, ls, m, maxit, A=None, b=None):
    if key not in _oracle:
        runs = []
        for p, x0 in enumerate(X0):
            if A is not None:
                O.dense_set(A[p], b[p])
            runs.append(O.lbfgs(obj, x0, ls, m, maxit, 1e-5, mode=O.CANON))
        _oracle[key] = runs
    return _oracle[key]


# ---- 1. stencil objectives: padded rows and packed tensors, apart and in place ------------------------
FORMS = ["rows", "packed", "rows_in_place", "packed_in_place"]
STENCIL = []
for oi, obj in enumerate(OBJS):
    for fi, form in enumerate(FORMS):
        STENCIL.append((obj, form, SEARCHES[(oi + fi) % 4], [1, 5][(oi + fi) % 2]))
assert {s for o, f, s, m in STENCIL} == set(SEARCHES)


@pytest.mark.parametrize("obj,form,ls,m", STENCIL)
def test_padded_rows_and_packed(obj, form, ls, m):
    maxit = 12
    X0 = x0s(SIZES)
    orc = oracle(("stencil", obj, ls, m), obj, X0, ls, m, maxit)
    assert len(set(o["iters"] for o in orc)) >= 2  # a condition on the inputs (CPU)
    kind = "packed" if form.startswith("packed") else "rows"
    xin = Buf(X0, kind, NAN)
    out = xin if form.endswith("in_place") else Buf([np.full(n, SENTINEL) for n in SIZES], kind, SENTINEL)
    if kind == "rows":
        assert xin.view.shape == (len(SIZES), max(SIZES) + 3) and xin.view.storage_offset() == 1
    with L.Batch(SIZES, m) as bt:
        rh = bt.minimize(obj, X0, ls, max_iterations=maxit, tolerance=1e-5, trace=True)
        rd = bt.minimize_device(obj, xin.view, ls, max_iterations=maxit, tolerance=1e-5, trace=True, out=out.view)
        assert rd["x"] is out.view
        if out is not xin:  # out=None gives the input's form
            rn = bt.minimize_device(obj, xin.view, ls, max_iterations=maxit, tolerance=1e-5, trace=True)
            assert rn["x"].shape == xin.view.shape and rn["x"].is_contiguous()
            got = host(rn["x"])
            cuts = np.cumsum([0] + SIZES)
            for p, n in enumerate(SIZES):
                assert same_bits(got[cuts[p]:cuts[p + 1]] if kind == "packed" else got[p, :n], rh["x"][p]), (form, p)
    assert out.outside_unchanged(), (obj, form)
    if out is not xin:
        assert xin.outside_unchanged() and all(same_bits(a, b) for a, b in zip(xin.parts(), X0))  # x0 is only read
    r = with_host_x(rd, out)
    same_result(r, rh, (obj, form, ls, m))
    for p in range(len(SIZES)):
        check_problem(r, p, orc[p], (obj, form, ls, m))


# ---- 2. dense quadratics by reference ---------------------------------------------------------------------
def spd(n, seed):
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    M = (Q * np.logspace(0, 3, n)) @ Q.T
    return (M + M.T) / 2, rs.uniform(-1.0, 1.0, n), O.x0_uniform(n, seed, -2.0, 2.0)


def dense_data():
    A, b, X0 = zip(*[spd(n, 4000 + n) for n in DSIZES])
    return list(A), list(b), list(X0)


DENSE_FORMS = [("rows", "rows"), ("packed", "packed"), ("packed", "rows"), ("rows", "packed")]  # (A, b)


@pytest.mark.parametrize("fa,fb", DENSE_FORMS)
def test_dense_by_reference(fa, fb):
    i = DENSE_FORMS.index((fa, fb))
    ls, m, maxit = SEARCHES[i], [1, 5][i % 2], 14
    A1, b1, X0 = dense_data()
    A2, b2 = [0.5 * a + 0.5 * np.eye(len(a)) for a in A1], [2.0 * v for v in b1]
    orc1 = oracle(("dense", 1, ls, m), "dense", X0, ls, m, maxit, A1, b1)
    orc2 = oracle(("dense", 2, ls, m), "dense", X0, ls, m, maxit, A2, b2)
    At, bt_ = Buf(A1, fa, NAN), Buf(b1, fb, NAN)
    if fa == "rows":
        W = max(DSIZES) + 3
        assert At.view.stride() == (W * W + 5, W, 1)
    xin = Buf(X0, "rows", NAN)
    out = Buf([np.full(n, SENTINEL) for n in DSIZES], "packed", SENTINEL)
    kw = dict(max_iterations=maxit, tolerance=1e-5, trace=True)
    with L.Batch(DSIZES, m) as bt:
        bt.set_dense_quadratics_device(At.view, bt_.view)
        assert bt._dq_refs[0] is At.view and bt._dq_refs[1] is bt_.view
        rd = with_host_x(bt.minimize_device("dense", xin.view, ls, out=out.view, **kw), out)
        assert out.outside_unchanged()
        r_mixed = bt.minimize("dense", X0, ls, **kw)  # host x, referenced A
        # the same memory, other data, no setter call
        At2, bt2 = Buf(A2, fa, NAN), Buf(b2, fb, NAN)
        At.buf.copy_(At2.buf)
        bt_.buf.copy_(bt2.buf)
        r2 = with_host_x(bt.minimize_device("dense", xin.view, ls, out=out.view, **kw), out)
        bt.set_dense_quadratics(A1, b1)  # the host form: the batch's own packed copies
        assert bt._dq_refs is None
        rh = bt.minimize("dense", X0, ls, **kw)
    assert all(same_bits(a, b) for a, b in zip(At.parts(), A2)) and all(same_bits(a, b) for a, b in zip(bt_.parts(), b2))
    assert xin.outside_unchanged() and all(same_bits(a, b) for a, b in zip(xin.parts(), X0))
    same_result(rd, rh, (fa, fb, "host forms"))
    same_result(rd, r_mixed, (fa, fb, "host x, referenced A"))
    for p in range(len(DSIZES)):
        check_problem(rd, p, orc1[p], (fa, fb, "first data"))
        check_problem(r2, p, orc2[p], (fa, fb, "data overwritten in place"))


# ---- 3. few workgroups, in place ----------------------------------------------------------------------------
def test_two_workgroups_for_seven_problems_in_place():
    sizes, m, ls, obj = SIZES + [5], 3, "wolfe", "quad_tridiag"
    X0 = x0s(sizes)
    X0[1] = np.zeros(5)
    orc = oracle(("few",), obj, X0, ls, m, 25)
    assert len(set(o["iters"] for o in orc)) >= 3 and 0 in [o["iters"] for o in orc]  # a condition on the inputs (CPU)
    results = []
    for launch in [(0, 0), (2, 3)]:
        xin = Buf(X0, "rows", NAN)
        with L.Batch(sizes, m) as bt:
            bt.set_launch(*launch)
            res = bt.minimize_device(obj, xin.view, ls, max_iterations=25, trace=True, out=xin.view)
        assert res["x"] is xin.view and xin.outside_unchanged()
        r = with_host_x(res, xin)
        for p in range(len(sizes)):
            check_problem(r, p, orc[p], ("few", launch))
        results.append(r)
    assert results[1]["launches"] > results[0]["launches"]
    for k in RESULT_KEYS:
        assert same_bits(np.asarray(results[0][k], np.float64), np.asarray(results[1][k], np.float64)), k


# ---- 4. refusals: a status or an exception, nothing launched --------------------------------------------------
def test_refusals():
    sizes, m = [5, 3, 4], 2
    B, nmax, total = len(sizes), max(sizes), sum(sizes)
    A = [np.eye(n) * (p + 1.0) for p, n in enumerate(sizes)]
    b = [np.full(n, 0.5) for n in sizes]
    X0 = [O.x0_uniform(n, 1 + p, -2.0, 2.0) for p, n in enumerate(sizes)]
    orc = oracle(("refuse",), "dense", X0, "backtracking", m, 50, A, b)
    lib, k = L.lib(), L.constants()
    ROS, DENSE_OBJ, BT, PK = L.OBJECTIVES["rosenbrock"], L.OBJECTIVES["dense"], L.LINE_SEARCHES["backtracking"], L.BATCH_PACKED
    with L.Batch(sizes, m) as bt:
        xin = Buf(X0, "rows", NAN)
        xpk = Buf(X0, "packed", NAN)
        out = Buf([np.full(n, SENTINEL) for n in sizes], "rows", SENTINEL)
        opk = Buf([np.full(n, SENTINEL) for n in sizes], "packed", SENTINEL)
        At, bt_ = Buf(A, "rows", NAN), Buf(b, "rows", NAN)
        Apk, bpk = Buf(A, "packed", NAN), Buf(b, "packed", NAN)
        ld, W = xin.ld, At.lda
        pinned = torch.full((B * W * W + 64,), 1.0, dtype=torch.float64).pin_memory()
        assert pinned.is_pinned()
        before = [host(t.buf) for t in (xin, xpk, out, opk, At, Apk)]

        def untouched():
            return all(same_bits(host(t.buf), h) for t, h in zip((xin, xpk, out, opk, At, Apk), before))

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

        X, Y, XP, YP = xin.view.data_ptr(), out.view.data_ptr(), xpk.view.data_ptr(), opk.view.data_ptr()
        AP, BP, APK, BPK = At.view.data_ptr(), bt_.view.data_ptr(), Apk.view.data_ptr(), bpk.view.data_ptr()
        # strides, at the C level: a row stride under the largest n, one x0 for all, other negatives
        for ldx0 in (nmax - 1, 0, -2, -nmax):
            c_minimize(X, ldx0, Y, ld)
        for ldx in (nmax - 1, 0, -2):
            c_minimize(X, ld, Y, ldx)
        c_minimize(None, PK, Y, ld)
        c_minimize(X, ld, Y, ld, obj=DENSE_OBJ)  # dense before any data is set
        c_setter(APK, PK, W, BPK, PK)  # A packed with lda given
        c_setter(APK, W * W, PK, BPK, PK)
        c_setter(AP, 0, W, BP, ld)  # no shared A, no shared b
        c_setter(AP, W * W + 5, W, BP, 0)
        c_setter(AP, W * W + 5, nmax - 1, BP, ld)
        c_setter(AP, (nmax - 1) * W + nmax - 1, W, BP, ld)
        c_setter(AP, W * W + 5, W, BP, nmax - 1)
        c_setter(None, PK, PK, BPK, PK)
        # pinned host memory is visible to the device: refused by its kind, not found out by a fault
        P = pinned.data_ptr()
        c_minimize(P, PK, Y, ld)
        c_minimize(X, ld, P, PK)
        c_setter(P, PK, PK, BPK, PK)
        c_setter(APK, PK, PK, P, ld)
        assert bool((pinned == 1.0).all())
        # a packed buffer one element short of the sum of the sizes: the allocation-range check. The
        # allocations are the runtime's own, of exactly that many bytes (a caching allocator's blocks are larger).
        rt = C.CDLL(L.hip_runtimes()[0])
        rt.hipMalloc.argtypes, rt.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        short_x, short_a = C.c_void_p(), C.c_void_p()
        assert rt.hipMalloc(C.byref(short_x), 8 * (total - 1)) == 0
        assert rt.hipMalloc(C.byref(short_a), 8 * (sum(n * n for n in sizes) - 1)) == 0
        try:
            c_minimize(short_x.value, PK, Y, ld)
            c_minimize(X, ld, short_x.value, PK)
            c_setter(short_a.value, PK, PK, BPK, PK)
            c_setter(APK, PK, PK, short_x.value, PK)
        finally:
            assert rt.hipFree(short_x) == 0 and rt.hipFree(short_a) == 0
        c_minimize(X, ld, Y, ld, obj=DENSE_OBJ)  # a refused setter sets nothing
        # the binding: shapes and strides raise before the library is called
        refused(ValueError, bt.minimize_device, "rosenbrock", xin.buf.as_strided((B, nmax), (nmax - 1, 1), 1))
        refused(ValueError, bt.minimize_device, "rosenbrock", xin.view[:, :nmax - 1])
        refused(ValueError, bt.minimize_device, "rosenbrock", xin.view[:2])
        refused(ValueError, bt.minimize_device, "rosenbrock", xin.view[:1].expand(B, ld))  # one x0 for all
        refused(ValueError, bt.minimize_device, "rosenbrock", xpk.view[:-1])
        refused(ValueError, bt.minimize_device, "rosenbrock", xpk.buf[::2][:total])
        refused(ValueError, bt.minimize_device, "rosenbrock", xin.view, out=opk.view[:-1])
        refused(ValueError, bt.minimize_device, "rosenbrock", xin.view.cpu())
        refused(TypeError, bt.minimize_device, "rosenbrock", xin.view.float())
        refused(TypeError, bt.minimize_device, "rosenbrock", X0)
        refused(ValueError, bt.set_dense_quadratics_device, At.view[:, :, :nmax - 1], bt_.view)
        refused(ValueError, bt.set_dense_quadratics_device, At.view.transpose(1, 2), bt_.view)
        refused(ValueError, bt.set_dense_quadratics_device, At.view[:1].expand(B, W, W), bt_.view)  # one A for all
        refused(ValueError, bt.set_dense_quadratics_device, Apk.view[:-1], bpk.view)
        refused(ValueError, bt.set_dense_quadratics_device, Apk.view, bpk.view[:-1])
        refused(TypeError, bt.set_dense_quadratics_device, Apk.view.float(), bpk.view)
        refused(L.LbfgsError, bt.minimize_device, "dense", xin.view, out=out.view)
        # overlaps: x over x0 other than identically (a packed x over padded x0 rows), x over the referenced A and b
        refused(L.LbfgsError, bt.minimize_device, "rosenbrock", xin.view, out=xin.buf[2:2 + total])
        refused(L.LbfgsError, bt.minimize_device, "rosenbrock", xpk.view, out=xpk.buf[:total])
        bt.set_dense_quadratics_device(Apk.view, bt_.view)
        refused(L.LbfgsError, bt.minimize_device, "dense", xin.view, out=Apk.view[:total])
        refused(L.LbfgsError, bt.minimize_device, "dense", xin.view, out=Apk.buf[-total - 1:-1])  # the last matrix's tail
        refused(L.LbfgsError, bt.minimize_device, "dense", xin.view, out=bt_.view)
        # and the batch still works
        res = with_host_x(bt.minimize_device("dense", xin.view, "backtracking", max_iterations=50, trace=True, out=out.view), out)
        assert out.outside_unchanged()
        for p in range(B):
            check_problem(res, p, orc[p], "after refusals")
