"""CPU-side checks of the batched solver's boundary (no GPU): lbfgs_batch_plan's limits and byte
count, and the new names in the binding and the library."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-lbfgs_amd")
sys.path.insert(0, PKG)
import lbfgs_amd as L  # noqa: E402

BATCH_SYMBOLS = ["lbfgs_batch_plan", "lbfgs_batch_create", "lbfgs_batch_destroy", "lbfgs_batch_last_error",
                 "lbfgs_batch_set_launch", "lbfgs_batch_minimize", "lbfgs_batch_trace_len",
                 "lbfgs_batch_trace_get", "lbfgs_batch_events_get"]


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)


@pytest.mark.parametrize("n,m,batch", [(1, 1, 1), (32768, 16, 1), (5, 5, 4096)])
def test_plan_accepts(n, m, batch):
    _ensure_built()
    assert L.plan(n, m, batch) > 0


@pytest.mark.parametrize("n,m,batch", [(0, 5, 1), (32769, 5, 1), (100, 0, 1), (100, 17, 1), (100, 5, 0)])
def test_plan_rejects(n, m, batch):
    _ensure_built()
    with pytest.raises(L.LbfgsError) as e:
        L.plan(n, m, batch)
    assert e.value.rc == -1  # LBFGS_ERR_BAD_ARG
    # the C entry point itself, with and without the byte count
    b = ctypes.c_double(-1.0)
    assert L.lib().lbfgs_batch_plan(n, m, batch, ctypes.byref(b)) == -1
    assert L.lib().lbfgs_batch_plan(n, m, batch, None) == -1
    assert b.value == -1.0


def test_plan_bytes_linear_in_batch():
    _ensure_built()
    for n, m in [(5, 2), (10_000, 5), (32768, 16)]:
        one = L.plan(n, m, 1)
        # at least the vectors the solver keeps per problem: x, g, xn, gn, d, q, r and m + 1 pairs
        assert one >= 8 * n * (7 + 2 * (m + 1))
        for b in (2, 7, 256, 4096):
            assert L.plan(n, m, b) == b * one


def test_new_names_exported():
    _ensure_built()
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in BATCH_SYMBOLS:
        assert s in L.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert callable(L.plan) and hasattr(L.Batch, "minimize") and hasattr(L.Batch, "set_launch")
