"""CPU-side checks of the dense batch's boundary (no GPU): lbfgs_batch_dense_plan's limits and byte
count, and the two new prototypes in the public header."""
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

NMAX = 4096  # the dense batch's limit on n (include/lbfgs_hip.h)


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)


@pytest.mark.parametrize("n,m,batch", [(1, 1, 1), (NMAX, 16, 1), (5, 5, 4096), (500, 5, 1024)])
@pytest.mark.parametrize("shared", [False, True])
def test_plan_accepts(n, m, batch, shared):
    _ensure_built()
    assert L.plan_dense(n, m, batch, shared) > L.plan(n, m, batch)
    assert L.lib().lbfgs_batch_dense_plan(n, m, batch, int(shared), None) == 0


@pytest.mark.parametrize("n,m,batch", [(0, 5, 1), (NMAX + 1, 5, 1), (100, 0, 1), (100, 17, 1), (100, 5, 0)])
@pytest.mark.parametrize("shared", [0, 1])
def test_plan_rejects(n, m, batch, shared):
    _ensure_built()
    with pytest.raises(L.LbfgsError) as e:
        L.plan_dense(n, m, batch, bool(shared))
    assert e.value.rc == -1  # LBFGS_ERR_BAD_ARG
    # the C entry point itself, with and without the byte count
    b = ctypes.c_double(-1.0)
    assert L.lib().lbfgs_batch_dense_plan(n, m, batch, shared, ctypes.byref(b)) == -1
    assert L.lib().lbfgs_batch_dense_plan(n, m, batch, shared, None) == -1
    assert b.value == -1.0


def test_plan_bytes_grow_by_the_matrices():
    """Unshared, every problem adds its own n x n matrix; shared, the whole batch adds one. What is
    left per problem beyond the plain batch (the terms t, the trial gradient gt, b) is the same in
    both and holds at least three n-vectors."""
    _ensure_built()
    for n, m in [(1, 1), (5, 2), (500, 5), (NMAX, 16)]:
        for B in (1, 2, 7, 256, 1024):
            own, shared, plain = L.plan_dense(n, m, B), L.plan_dense(n, m, B, shared=True), L.plan(n, m, B)
            assert own - shared == (B - 1) * n * n * 8
            extra = shared - plain - n * n * 8
            assert extra == own - plain - B * n * n * 8
            assert extra >= B * 3 * n * 8 and extra == B * (L.plan_dense(n, m, 1) - L.plan(n, m, 1) - n * n * 8)


def test_prototypes_in_the_header_and_names_exported():
    _ensure_built()
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lbfgs_hip.h")).read())
    assert ("int lbfgs_batch_dense_plan(int64_t n, int m, int batch, int shared_A, double* bytes);") in src
    assert ("int lbfgs_batch_set_dense_quadratics(lbfgs_batch* b, const double* A, int shared_A, "
            "const double* bvec);") in src
    assert "#define LBFGS_HIP_ABI_VERSION 3" in src
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in ("lbfgs_batch_dense_plan", "lbfgs_batch_set_dense_quadratics"):
        assert s in L.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert callable(L.plan_dense) and hasattr(L.Batch, "set_dense_quadratics")
