"""CPU-side checks of the ragged batch's boundary (no GPU): the header declares
lbfgs_batch_ragged_plan, lbfgs_batch_create_ragged, lbfgs_batch_sizes and LBFGS_BATCH_PACKED and the
library exports them; the plan's limits and its byte count, which is per problem what
lbfgs_batch_plan(n_p, m, 1) gives plus the problem's share of the table (a row of six 64-bit values
and a 4-byte entry of the order of work: TABLE_BYTES), and with `dense` also t, gt, b and the matrix,
that is what lbfgs_batch_dense_plan(n_p, m, 1, 0) adds."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-lbfgs_amd")
sys.path.insert(0, PKG)
import lbfgs_amd as L  # noqa: E402

RAGGED_SYMBOLS = ["lbfgs_batch_ragged_plan", "lbfgs_batch_create_ragged", "lbfgs_batch_sizes"]
TABLE_BYTES = 6 * 8 + 4
BAD_ARG = -1


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)


def _c_plan(sizes, m, dense, batch=None):
    arr = (ctypes.c_int64 * max(len(sizes), 1))(*sizes)
    b = ctypes.c_double(-1.0)
    rc = L.lib().lbfgs_batch_ragged_plan(arr, len(sizes) if batch is None else batch, m, dense, ctypes.byref(b))
    return rc, b.value


def test_header_declares_and_library_exports():
    _ensure_built()
    src = open(os.path.join(ROOT, "include", "lbfgs_hip.h")).read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in RAGGED_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", src), s
        assert hasattr(lib, s), s
        assert s in L.EXPORTED_SYMBOLS, s
    assert re.search(r"#define\s+LBFGS_BATCH_PACKED\s+\(-1\)", src)
    assert L.BATCH_PACKED == -1 and callable(L.plan_ragged)


@pytest.mark.parametrize("sizes,m,dense", [([1], 1, 0), ([32768, 1, 513], 16, 0), ([4096, 2], 5, 1), ([5] * 4096, 5, 0)])
def test_plan_accepts(sizes, m, dense):
    _ensure_built()
    rc, b = _c_plan(sizes, m, dense)
    assert rc == 0 and b > 0
    assert L.plan_ragged(sizes, m, dense=bool(dense)) == b
    assert L.lib().lbfgs_batch_ragged_plan((ctypes.c_int64 * len(sizes))(*sizes), len(sizes), m, dense, None) == 0


@pytest.mark.parametrize("sizes,m,dense", [([5, 0], 5, 0), ([32769, 5], 5, 0), ([5, 4097], 5, 1), ([5, -3], 5, 0),
                                           ([5, 6], 0, 0), ([5, 6], 17, 0)])
def test_plan_rejects(sizes, m, dense):
    _ensure_built()
    rc, b = _c_plan(sizes, m, dense)
    assert rc == BAD_ARG and b == -1.0  # the byte count is left alone
    with pytest.raises(L.LbfgsError) as e:
        L.plan_ragged(sizes, m, dense=bool(dense))
    assert e.value.rc == BAD_ARG


def test_plan_rejects_empty_and_null():
    _ensure_built()
    assert _c_plan([5, 6], 5, 0, batch=0) == (BAD_ARG, -1.0)
    assert _c_plan([5, 6], 5, 0, batch=-1) == (BAD_ARG, -1.0)
    b = ctypes.c_double(-1.0)
    assert L.lib().lbfgs_batch_ragged_plan(None, 2, 5, 0, ctypes.byref(b)) == BAD_ARG and b.value == -1.0
    # 4097 is within the stencil limits, over the dense ones
    assert _c_plan([4097], 5, 0)[0] == 0 and _c_plan([4097], 5, 1)[0] == BAD_ARG


@pytest.mark.parametrize("m", [1, 5, 16])
def test_plan_bytes_are_the_sum_over_problems_plus_the_table(m):
    _ensure_built()
    sizes = [513, 5, 1537, 512, 129, 1024, 4096, 1]
    rc, b = _c_plan(sizes, m, 0)
    assert rc == 0 and b == sum(L.plan(n, m, 1) for n in sizes) + TABLE_BYTES * len(sizes)
    rc, bd = _c_plan(sizes, m, 1)
    assert rc == 0 and bd == sum(L.plan_dense(n, m, 1) for n in sizes) + TABLE_BYTES * len(sizes)
    assert bd - b >= sum(8 * (n * n + 3 * n) for n in sizes)  # the matrices, and b, t and gt


@pytest.mark.parametrize("n,m,B", [(513, 3, 4), (5, 1, 300), (32768, 16, 2)])
def test_all_equal_sizes_differ_from_the_uniform_plan_by_the_table(n, m, B):
    _ensure_built()
    assert L.plan_ragged([n] * B, m) == L.plan(n, m, B) + TABLE_BYTES * B
    if n <= L.DENSE_BATCH_NMAX:
        assert L.plan_ragged([n] * B, m, dense=True) == L.plan_dense(n, m, B) + TABLE_BYTES * B


def test_sizes_and_create_refuse_null():
    _ensure_built()
    lib = L.lib()
    n_out, off = (ctypes.c_int64 * 2)(7, 7), (ctypes.c_int64 * 3)(7, 7, 7)
    assert lib.lbfgs_batch_sizes(None, n_out, off) == BAD_ARG
    assert lib.lbfgs_batch_sizes(None, None, None) == BAD_ARG
    assert list(n_out) == [7, 7] and list(off) == [7, 7, 7]
    # the creator refuses before it touches a device: no handle, bad sizes, no sizes
    h = ctypes.c_void_p(1)
    good = (ctypes.c_int64 * 2)(5, 6)
    assert lib.lbfgs_batch_create_ragged(None, good, 5, 2, 0) == BAD_ARG
    for arr, m, batch in [((ctypes.c_int64 * 2)(5, 0), 5, 2), ((ctypes.c_int64 * 2)(5, 32769), 5, 2), (good, 17, 2),
                          (good, 5, 0), (None, 5, 2)]:
        h.value = 1
        assert lib.lbfgs_batch_create_ragged(ctypes.byref(h), arr, m, batch, 0) == BAD_ARG
        assert h.value is None
