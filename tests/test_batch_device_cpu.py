"""CPU-side checks of the batch's device-memory forms (no GPU): the two prototypes in the public
header, the unchanged ABI version, the exported names, the refusal of a NULL batch, and the two
methods of Batch."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-lbfgs_amd")
sys.path.insert(0, PKG)
import lbfgs_amd as L  # noqa: E402

NAMES = ("lbfgs_batch_minimize_device", "lbfgs_batch_set_dense_quadratics_device")
BAD_ARG = -1


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)


def test_prototypes_in_the_header_and_abi_version():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lbfgs_hip.h")).read())
    assert ("int lbfgs_batch_minimize_device(lbfgs_batch* b, int objective, int line_search, "
            "const lbfgs_constants* k, const double* x0_dev, int64_t ldx0, double* x_out_dev, int64_t ldx, "
            "int max_iterations, double tolerance, unsigned flags, lbfgs_result* out);") in src
    assert ("int lbfgs_batch_set_dense_quadratics_device(lbfgs_batch* b, const double* A_dev, "
            "int64_t a_batch_stride, int64_t lda, const double* b_dev, int64_t ldb);") in src
    assert "#define LBFGS_HIP_ABI_VERSION 3 " in src


def test_names_exported():
    _ensure_built()
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in NAMES:
        assert s in L.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s


def test_null_batch_is_bad_arg():
    _ensure_built()
    lib = L.lib()
    k = L.constants()
    res = L.Result()
    assert lib.lbfgs_batch_minimize_device(None, L.OBJECTIVES["rosenbrock"], L.LINE_SEARCHES["backtracking"],
                                           ctypes.byref(k), None, 5, None, 5, 10, 1e-5, 0, ctypes.byref(res)) == BAD_ARG
    assert lib.lbfgs_batch_set_dense_quadratics_device(None, None, 25, 5, None, 5) == BAD_ARG


def test_batch_has_the_two_methods():
    assert callable(getattr(L.Batch, "minimize_device", None))
    assert callable(getattr(L.Batch, "set_dense_quadratics_device", None))
